"""The depth-output march's part of the launch plan (csrc/host/launch_plan.hpp plan_depth_output), its known-answer row (csrc/host/ray_query.hpp) and the commit
plan's row of the frame kinds on the CPU: the new kind appended last; taken exactly where depth_output.active says, in front of the depth limit's line - the
depth limit alone still plans DepthLimitedMarch, both together plan the new kind with `limited` - and every other plan kept member for member; the LDS size, the
row's refusals and record size against literals.  Then the code objects of the built library: 144 new kernels, none with a private segment or a spilled vector
register.  The driver (tests/depth_output_plan_driver.cpp) holds the tables; no GPU, no ROCm headers."""
import itertools
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")
CSRC = os.path.join(ROOT, "open-volume-renderer_amd", "csrc")
SCENARIOS = ["variants", "precedence", "query_row", "commit_row"]
KIND_DEPTH_LIMITED, KIND_DEPTH_OUTPUT = 11, 12      # FrameKind's numbers: the new kind is the last


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("depth_output_plan") / "driver"
    # (no ROCm include path: the plans must not need one)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HOST, "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "depth_output_plan_driver.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_driver_runs_every_scenario_listed_here(driver):
    assert subprocess.check_output([driver, "--list"], text=True).split() == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_scenario(driver, scenario):
    p = subprocess.run([driver, scenario], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr


def test_the_plans_rule_is_the_models_over_the_whole_matrix(ovr, driver):
    """modes x frame kinds x shadings x pre-integration x gradient opacity x depth limit: the planned kind is the new one exactly where depth_output.active
    says, `limited` exactly where the depth limit's own rule would draw"""
    D, M = ovr.depth_output, ovr.max_depth
    n = taken = 0
    for on, slices, iso, proj, shading, pre, gradop, md in itertools.product((0, 1), (0, 1), (0, 2), (0, 1, 3), (0, 1, 2), (0, 1), (0, 1), (0, 1)):
        kind, limited = (int(v) for v in subprocess.check_output([driver, "rule"] + [str(v) for v in (on, slices, iso, proj, shading, pre, gradop, md)], text=True).split())
        want = D.active(on, shading, slices, iso, proj, pre, gradop)
        assert (kind == KIND_DEPTH_OUTPUT) == want, (on, slices, iso, proj, shading, pre, gradop, md, kind)
        assert limited == int(want and md == 1) == int(D.limited(on, md == 1, (4, 3), (4, 3), shading=shading, slices=slices, isovalues=iso, projection_mode=proj, preintegration=pre,
                                                                 gradient_opacity_mode=gradop))
        if not want:      # the depth limit's own kind where its own rule says so
            assert (kind == KIND_DEPTH_LIMITED) == M.active(md == 1, (4, 3), (4, 3), shading, slices, iso, proj, pre, gradop)
        n += 1
        taken += want
    assert n == 2 * 2 * 2 * 3 * 3 * 2 * 2 * 2 and taken == 3 * 2


def test_the_setter_is_recorded_with_the_frame_kinds():
    api = open(os.path.join(CSRC, "ovr_hip_api.cpp")).read()
    assert "if (r->depth_output.update())" in api and "GROUP_FORWARD(r, ovr_hip_set_depth_output(m, mode, threshold));" in api
    body = api.split("int ovr_hip_set_depth_output(")[1].split("\n}\n")[0]
    assert body.index("depth_output_check(") < body.index("r->depth_output.set(")      # validated before anything changes
    plan = open(os.path.join(HOST, "commit_plan.hpp")).read()
    assert "ovr_hip_set_depth_output" in plan


def test_the_kernel_sources_of_the_parent_are_untouched():
    """the depth-output kernel lives in files of its own and calls the march's functions: no existing kernel source names it"""
    for name in ("ovr_hip_device.h", "ovr_hip_slices.h", "ovr_hip_slice_context.h", "ovr_hip_isosurface_context.h", "ovr_hip_isosurface_ao.h", "ovr_hip_preintegration.h", "ovr_hip_gradient_opacity.h",
                 "ovr_hip_max_depth.h", "ovr_hip_march.hip", "ovr_hip_slices.hip", "ovr_hip_isosurface.hip", "ovr_hip_preintegration.hip", "ovr_hip_gradient_opacity.hip", "ovr_hip_max_depth.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert "depth_output" not in text and "depth_tau" not in text, name
    new = open(os.path.join(CSRC, "ovr_hip_depth_output.h")).read()
    for call in ("stage_tf(", "tf_alpha<true>(", "opacity_correction<false>(", "tf_color(", "shade_light<true, ORTHO>(", "shade_factor<true>(", "assign_pixel_quad(", "slice_sample_position(",
                 "write_pixel(", "store_block_counters(", "__ballot(", "gradient_difference<VT, AM>(", "max_depth_cut("):
        assert call in new, call
    assert new.count("amdgpu_waves_per_eu(1, kMarchWavesPerEu)") == 2
    # at most one depth load per pixel, in front of the samples' loop, and none without an image
    kernel = new.split("void depth_output_kernel(")[1].split("void depth_output_floats_kernel(")[0]
    assert kernel.count("P.max_depth[") == 1 and kernel.index("P.max_depth[") < kernel.index("for (int k_spp") and "P.max_depth) ? P.max_depth[" in kernel
    # tau stands behind everything else in the kernels' parameters
    params = open(os.path.join(CSRC, "ovr_hip_kernels.h")).read().split("struct RayMarchParams {")[1].split("\n};")[0]
    assert params.rstrip().endswith("float depth_tau;")


def test_no_depth_output_kernel_has_a_private_segment():
    """No new kernel may use scratch: every depth-output kernel of the built library reports a private segment of 0 bytes and no spilled vector register - read
    from the code objects embedded in the library by tools/kernel_metadata.py (no GPU, no recompilation).  The VGPR counts are printed beside the depth-limited
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
    mine = {n: k for n, k in kernels.items() if "depth_output_kernel" in n or "depth_output_floats_kernel" in n}
    neighbour = {n: k for n, k in kernels.items() if "max_depth_kernel" in n or "max_depth_floats_kernel" in n}
    # 5 types x their addressing modes (f32: 0 ... 3; the 16- and 8-bit types: 0 ... 4) x (2 shading modes x 2 cameras + 2 known-answer twins)
    assert len(mine) == (4 + 4 * 5) * 6 == 144 == len(neighbour), (len(mine), len(neighbour))
    for shade in (0, 1):
        # (per shading mode: the GRADIENT kernels carry the gradient taps)
        print("VGPRs, shading", shade, ": depth_output_kernel", KM.rng(sorted(k[".vgpr_count"] for n, k in mine.items() if "floats" not in n and _shade(n) == shade)),
              "max_depth_kernel", KM.rng(sorted(k[".vgpr_count"] for n, k in neighbour.items() if "floats" not in n and _shade(n) == shade)))
    print("VGPRs: depth_output_floats_kernel", KM.rng(sorted(k[".vgpr_count"] for n, k in mine.items() if "floats" in n)),
          "max_depth_floats_kernel", KM.rng(sorted(k[".vgpr_count"] for n, k in neighbour.items() if "floats" in n)))
    bad = {n: k for n, k in mine.items() if k[".private_segment_fixed_size"] != 0 or k[".vgpr_spill_count"] != 0}
    assert not bad, (len(bad), list(bad.items())[:3])


def _shade(mangled):
    """the SHADE template argument of a mangled kernel name: ...ILi<VT>ELi<AM>ELi<SHADE>E..."""
    import re
    m = re.search(r"ILi\d+ELi\d+ELi(\d+)E", mangled)
    return int(m.group(1)) if m else -1
