"""OVR_HIP_ISO_OPACITIES as the plugin parses it (plugin/isovalues_env.hpp parse_iso_opacities) on the CPU: one opacity in (0, 1] per isovalue of
OVR_HIP_ISOVALUES, separated by single commas, the whole string consumed - another count, a value outside (0, 1] or trailing text is an error, never a
shorter list."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_opacities_variable_is_parsed_whole(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "plugin"), os.path.join(ROOT, "tests", "iso_opacities_env_driver.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    src = open(os.path.join(ROOT, "plugin", "device_hip.cpp")).read()
    assert "ovrhip_plugin::parse_iso_opacities(ov, a, n) != n" in src and 'std::getenv("OVR_HIP_ISO_OPACITIES")' in src and "ovr_hip_set_isosurface_layers(h, v, a, n)" in src
