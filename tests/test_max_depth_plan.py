"""The depth-limited march's part of the launch plan (csrc/host/launch_plan.hpp plan_max_depth), its known-answer row (csrc/host/ray_query.hpp) and the commit
plan's row of the frame kinds on the CPU: the variant table, the kind taken exactly under the march with shading NONE or GRADIENT and neither an active
pre-integration nor an active gradient opacity - FULL shading, slices, isovalues, projections, pre-integration and gradient opacity keep their plans member for
member -, the LDS size, the row's refusals and record size against literals.  Then the code objects of the built library: 144 new kernels, none with a private
segment or a spilled vector register.  The driver (tests/max_depth_plan_driver.cpp) holds the tables; no GPU, no ROCm headers."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")
SCENARIOS = ["variants", "precedence", "query_row", "commit_row"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("max_depth_plan") / "driver"
    # (no ROCm include path: the plans must not need one)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HOST, "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "max_depth_plan_driver.cpp"), "-o", str(exe)])
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
    assert "if (r->max_depth.update())" in api and "ch.note(kShading, true, true);" in api
    assert "std::swap(r->d_max_depth, r->d_max_depth_queued)" in api      # the commit swaps the queued image in
    assert "group_call(r, [=](ovr_hip_renderer* m) { return set_max_depth_one(m, host, width, height); }" in api      # a group forwards the whole image
    assert "finish_frame_one(r)" in api.split("int set_max_depth_one(")[1].split("\n}\n")[0]      # the frame in flight is resolved before the copy
    plan = open(os.path.join(HOST, "commit_plan.hpp")).read()
    assert "ovr_hip_set_max_depth" in plan


def test_the_rule_is_read_from_the_host_header():
    frame = open(os.path.join(HOST, "frame.cpp")).read()
    plan = open(os.path.join(HOST, "launch_plan.hpp")).read()
    assert "max_depth_active(" in frame and "max_depth_size_matches(" in frame and "max_depth_active(" in plan and '#include "max_depth_host.hpp"' in plan
    assert "constexpr bool max_depth_active(" not in frame and "constexpr bool max_depth_active(" not in plan


def test_the_kernel_sources_of_the_parent_are_untouched():
    """the depth-limited kernel lives in files of its own and calls the march's functions: no existing kernel source names it"""
    csrc = os.path.join(ROOT, "open-volume-renderer_amd", "csrc")
    for name in ("ovr_hip_device.h", "ovr_hip_slices.h", "ovr_hip_slice_context.h", "ovr_hip_isosurface_context.h", "ovr_hip_isosurface_ao.h", "ovr_hip_preintegration.h", "ovr_hip_gradient_opacity.h",
                 "ovr_hip_march.hip", "ovr_hip_slices.hip", "ovr_hip_isosurface.hip", "ovr_hip_preintegration.hip", "ovr_hip_gradient_opacity.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert "max_depth" not in text, name
    new = open(os.path.join(csrc, "ovr_hip_max_depth.h")).read()
    for call in ("stage_tf(", "tf_alpha<true>(", "opacity_correction<false>(", "tf_color(", "shade_light<true, ORTHO>(", "shade_factor<true>(", "assign_pixel_quad(", "slice_sample_position(",
                 "write_pixel(", "store_block_counters(", "__ballot(", "gradient_difference<VT, AM>("):
        assert call in new, call
    assert "amdgpu_waves_per_eu(1, kMarchWavesPerEu)" in new
    # one depth load per pixel, in front of the samples' loop
    kernel = new.split("void max_depth_kernel(")[1].split("void max_depth_floats_kernel(")[0]
    assert kernel.count("P.max_depth[") == 1 and kernel.index("P.max_depth[") < kernel.index("for (int k_spp")


def test_no_depth_limited_kernel_has_a_private_segment():
    """No new kernel may use scratch: every depth-limited kernel of the built library reports a private segment of 0 bytes and no spilled vector register - read
    from the code objects embedded in the library by tools/kernel_metadata.py (no GPU, no recompilation).  The VGPR counts are printed beside the gradient-opacity
    kernel's, not asserted"""
    lib = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip.so")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_metadata as KM
    finally:
        sys.path.pop(0)
    if not (os.path.exists(lib) and os.path.exists(os.path.join(KM.LLVM, "llvm-objdump"))):
        pytest.skip("library or llvm tools not present")
    kernels = KM.read(lib, every=True)
    mine = {n: k for n, k in kernels.items() if "max_depth_kernel" in n or "max_depth_floats_kernel" in n}
    neighbour = {n: k for n, k in kernels.items() if "gradient_opacity_kernel" in n}
    # 5 types x their addressing modes (f32: 0 ... 3; the 16- and 8-bit types: 0 ... 4) x (2 shading modes x 2 cameras + 2 known-answer twins)
    assert len(mine) == (4 + 4 * 5) * 6 == 144, len(mine)
    print("VGPRs: max_depth_kernel", KM.rng(sorted(k[".vgpr_count"] for n, k in mine.items() if "floats" not in n)),
          "max_depth_floats_kernel", KM.rng(sorted(k[".vgpr_count"] for n, k in mine.items() if "floats" in n)),
          "gradient_opacity_kernel", KM.rng(sorted(k[".vgpr_count"] for k in neighbour.values())))
    bad = {n: k for n, k in mine.items() if k[".private_segment_fixed_size"] != 0 or k[".vgpr_spill_count"] != 0}
    assert not bad, (len(bad), list(bad.items())[:3])
