"""OVR_HIP_AO_SAMPLES / OVR_HIP_AO_DISTANCE as the plugin parses them (plugin/isovalues_env.hpp parse_ao) on the CPU: K an integer in 0 ... 16, the radius a float
above 0 or inf, each string consumed whole - anything else is an error and writes nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ao_variables_are_parsed_whole(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "plugin"), os.path.join(ROOT, "tests", "ambient_occlusion_env_driver.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    src = open(os.path.join(ROOT, "plugin", "device_hip.cpp")).read()
    assert 'std::getenv("OVR_HIP_AO_SAMPLES")' in src and 'std::getenv("OVR_HIP_AO_DISTANCE")' in src and "ovr_hip_set_ambient_occlusion(h, k, dist)" in src
    assert "ao_samples" not in src.replace("the scene's own ao_samples is not read", "")   # the scene's slot is not read in this change
