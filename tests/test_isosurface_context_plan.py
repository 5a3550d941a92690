"""The isosurface context's part of the launch plan (csrc/host/launch_plan.hpp plan_isosurface) and the commit plan's row of the frame kinds on the CPU: a
context plan is the clipped translucent plan plus the flag, with the transfer function's LDS and without skip or the AO twins; `error` on an oversized table;
slices keep their precedence and the mode is kept at n = 0; with the fact false every plan is what it was.  The driver
(tests/isosurface_context_plan_driver.cpp) holds the tables; no GPU, no ROCm headers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")
SCENARIOS = ["context", "precedence", "off_changes_nothing", "commit_row"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("isosurface_context_plan") / "driver"
    # (no ROCm include path: the plans must not need one)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HOST, os.path.join(ROOT, "tests", "isosurface_context_plan_driver.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_driver_runs_every_scenario_listed_here(driver):
    assert subprocess.check_output([driver, "--list"], text=True).split() == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_scenario(driver, scenario):
    p = subprocess.run([driver, scenario], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr


def test_the_setter_is_recorded_with_the_frame_kinds():
    api = open(os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "ovr_hip_api.cpp")).read()
    assert "set_ic = r->isosurface_context.update()" in api and "|| set_c || set_ic," in api
    assert "ovr_hip_set_isosurface_context" in open(os.path.join(HOST, "commit_plan.hpp")).read()


def test_the_kernel_sources_of_the_parent_are_untouched():
    """the context kernel lives in files of its own and calls the isosurface and march functions: no existing kernel source names it"""
    csrc = os.path.join(ROOT, "open-volume-renderer_amd", "csrc")
    for name in ("ovr_hip_device.h", "ovr_hip_slices.h", "ovr_hip_slice_context.h", "ovr_hip_isosurface_ao.h", "ovr_hip_march.hip", "ovr_hip_slices.hip", "ovr_hip_isosurface.hip",
                 "ovr_hip_slice_context.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert "isosurface_context" not in text and "iso_context" not in text, name
    new = open(os.path.join(csrc, "ovr_hip_isosurface_context.h")).read()
    code = "\n".join(line.split("//")[0] for line in new.splitlines())      # the statements, without the comments
    for call in ("iso_point<VT, AM, SHADE, false, true>(", "iso_step_events(sa, sb", "isosurface_colour(P, iso)", "slice_context_stage<VT, AM>(P, lds_raw", "opacity_correction<false>(",
                 "slice_sample_position(P, ix, iy"):
        assert call in code, call
    assert "iso_walk<" not in code      # the shadow ray is iso_point's own call of iso_walk: called, not copied


def test_no_context_kernel_has_a_private_segment():
    """No new kernel may use scratch: every isosurface_context kernel of the built library reports a private segment of 0 bytes and no spilled vector register -
    read from the code objects embedded in the library, as tests/test_abi.py reads the march kernels' (no GPU, no recompilation)"""
    lib = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip.so")
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(lib) and os.path.exists(os.path.join(llvm, "llvm-objdump"))):
        pytest.skip("library or llvm tools not present")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, capture_output=True, check=True)
        kernels, name = {}, None
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", f], cwd=tmp, capture_output=True, text=True, check=True).stdout
            for line in notes.splitlines():
                line = line.strip()
                if line.startswith(".name:"):
                    name = line.split(":", 1)[1].strip()
                    kernels[name] = {}
                elif name and line.split(":")[0] in (".private_segment_fixed_size", ".vgpr_spill_count", ".vgpr_count"):
                    k, v = line.split(":")
                    kernels[name][k.strip()] = int(v)
    mine = {n: k for n, k in kernels.items() if "isosurface_context" in n}
    assert len(mine) == 192, len(mine)      # 5 types x their addressing modes x (3 shading modes x 2 cameras + 2 known-answer twins)
    bad = {n: k for n, k in mine.items() if k[".private_segment_fixed_size"] != 0 or k[".vgpr_spill_count"] != 0}
    assert not bad, (len(bad), list(bad.items())[:3])
