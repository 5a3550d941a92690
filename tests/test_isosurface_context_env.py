"""OVR_HIP_ISO_CONTEXT as the plugin parses it (plugin/iso_context_env.hpp), through a stand-alone program built with the address and undefined-behaviour
sanitizers, as tests/test_slice_context_env.py holds OVR_HIP_SLICE_CONTEXT.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ["env_parser"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("isosurface_context_host") / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "plugin"),
                           os.path.join(ROOT, "tests", "isosurface_context_host_driver.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_driver_runs_every_scenario_listed_here(driver):
    assert subprocess.check_output([driver, "--list"], text=True).split() == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_parser_under_sanitizers(driver, scenario):
    p = subprocess.run([driver, scenario], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr


def test_the_plugin_is_rebuilt_with_the_parser_and_the_variable_is_documented():
    """(that the plugin calls the parser and the setter is held by behaviour: tests/test_isosurface_context_gpu.py runs the unmodified renderbatch with the variable)"""
    assert "iso_context_env.hpp" in open(os.path.join(ROOT, "plugin", "Makefile")).read()      # a dependency of libdevice_hip.so
    assert "OVR_HIP_ISO_CONTEXT" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
