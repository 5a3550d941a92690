"""OVR_HIP_ISOVALUES as the plugin parses it (plugin/isovalues_env.hpp) on the CPU: one to four values separated by single commas, the whole string consumed -
trailing text, a trailing comma, an empty field or a fifth value is an error, never a shorter list."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_isovalues_variable_is_parsed_whole(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "plugin"), os.path.join(ROOT, "tests", "isovalues_env_driver.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ovrhip_plugin::parse_isovalues(iv" in open(os.path.join(ROOT, "plugin", "device_hip.cpp")).read()
