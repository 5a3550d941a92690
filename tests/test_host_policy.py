"""The host state machine's automatic decisions (csrc/host/policy.hpp: layout rule, layout / pipeline tuner, automatic pipeline, adaptive
skipping, the small sizing rules) driven through scripted frame sequences on the CPU: the header is free of HIP, so the host compiler builds
host_policy_driver.cpp against it and every scenario of the driver is one test.  The expectations in the driver's tables are the rules as
DESIGN.md sections 2 / 4 and the comments in policy.hpp state them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")
SCENARIOS = ["layout_rule", "tuner_light", "tuner_heavy_close", "tuner_heavy_apart", "tuner_no_replicas", "tuner_forced_layout", "tuner_kept_decision",
             "tuner_recheck", "tuner_reset_and_off", "auto_pipeline", "skipping", "small_rules"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("host_policy") / "driver"
    # (no ROCm include path: the policies must not need one)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HOST, os.path.join(ROOT, "tests", "host_policy_driver.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_driver_runs_every_scenario_listed_here(driver):
    assert subprocess.check_output([driver, "--list"], text=True).split() == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_policy(driver, scenario):
    p = subprocess.run([driver, scenario], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
