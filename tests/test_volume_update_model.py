"""ovr_hip_update_volume without a GPU: the host arithmetic of csrc/host/update_extent.hpp - which bricks, rows, layers, quad
cells and macrocells hold a copy of a voxel of the box - against brute force (volume_update_driver.cpp, built by the host compiler against that
header alone), the macrocell set against the oracle's macrocell grid, and the entry point's null-handle answer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")

# Vox<>'s cx / mbx / by / bz / transposed of every bricked layout (ovr_hip_device.h) and lx / ly / lz of the quad replicas
BRICK = {"f32": (3, 10, 2, 1, 0), "u16_i16": (3, 10, 2, 2, 0), "u8_i8": (7, 4, 2, 2, 0), "f32_t": (1, 32, 2, 2, 0), "f32_tt": (1, 32, 2, 2, 1),
         "u16_t": (1, 32, 2, 3, 0), "u16_tt": (1, 32, 2, 3, 1)}
QUAD = {"f32_q": (1, 1, 1), "u16_q": (2, 1, 1), "u8_q": (2, 2, 1)}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("volume_update") / "driver"
    # (no ROCm include path: the header must not need one)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", HOST, os.path.join(ROOT, "tests", "volume_update_driver.cpp"), "-o", str(exe)])
    return str(exe)


def run(driver, *args):
    p = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr


def test_the_geometries_are_the_device_headers():
    """the numbers above are Vox<>'s: read from ovr_hip_device.h"""
    import re
    text = open(os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "ovr_hip_device.h")).read()
    found = {}
    for m in re.finditer(r"template <> struct Vox<VOX_(\w+)> \{(.*?)\n\};", text, re.S):
        body = m.group(2)
        g = re.search(r"cx = (\d+), mbx = (\d+), by = (\d+), bz = (\d+)", body)
        q = re.search(r"lx = (\d+), ly = (\d+), lz = (\d+)", body)
        found[m.group(1)] = (tuple(map(int, g.groups())), tuple(map(int, q.groups())) if q else None)
    assert found["F32"][0] + (0,) == BRICK["f32"] and found["U16"][0] == found["I16"][0] and found["U16"][0] + (0,) == BRICK["u16_i16"]
    assert found["U8"][0] == found["I8"][0] and found["U8"][0] + (0,) == BRICK["u8_i8"]
    assert found["F32_T"][0] + (0,) == BRICK["f32_t"] and found["U16_T"][0] + (0,) == BRICK["u16_t"]
    assert found["F32_Q"][1] == QUAD["f32_q"] and found["U16_Q"][1] == QUAD["u16_q"] and found["U8_Q"][1] == QUAD["u8_q"]


def test_the_box_set_holds_corners_faces_the_whole_grid_and_the_macrocell_edges(driver):
    run(driver, "boxes")


@pytest.mark.parametrize("layout", sorted(BRICK))
def test_brick_ranges_against_brute_force(driver, layout):
    run(driver, "brick", *BRICK[layout])


@pytest.mark.parametrize("layout", sorted(QUAD))
def test_quad_cell_ranges_against_brute_force(driver, layout):
    run(driver, "quad", *QUAD[layout])


def test_macrocell_ranges_against_brute_force(driver):
    run(driver, "cells")


def test_argument_checks(driver):
    run(driver, "args")


def predicted_cells(n, a, b):
    """update_extent.hpp macrocell_axis, restated: cell c reads the voxels [max(16 c - 1, 0), + 17) - voxel 16 belongs to cells 0 and 1"""
    return (0 if a <= 16 else a >> 4), min(b >> 4, (n + 15) // 16 - 1)


# (x0, x1, y0, y1, z0, z1): interior, a start at voxel 16 (cell 0's window reaches it), ends at 16 k - 1 / 16 k / 16 k + 1, a face, one voxel
MC_BOXES = [(20, 40, 9, 18, 13, 26), (16, 17, 16, 20, 16, 30), (3, 31, 5, 32, 7, 33), (47, 48, 48, 49, 49, 50), (0, 70, 60, 67, 0, 1), (69, 70, 66, 67, 68, 69),
            (17, 18, 33, 34, 1, 2)]


@pytest.mark.parametrize("box", MC_BOXES)
def test_macrocells_change_only_inside_the_predicted_cells_and_in_all_of_them(ovr, oracle, box):
    O = oracle
    x0, x1, y0, y1, z0, z1 = box
    v0 = ovr.synth.make_volume(0, np.float32, dims=(70, 67, 69))
    assert v0.shape == (69, 67, 70)
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 64, np.float32)
    cam = ovr.synth.make_camera("oblique", 70)
    mm0, _ = O.OracleScene(v0, colors, alphas, vr, cam, 8, 8).macrocells()
    lo, hi = zip(predicted_cells(70, x0, x1), predicted_cells(67, y0, y1), predicted_cells(69, z0, z1))
    inside = np.zeros(mm0.shape[:3], bool)
    inside[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    rng = np.random.default_rng(7)
    # values from V0's range: cells outside the predicted box keep their range
    v1 = v0.copy()
    v1[z0:z1, y0:y1, x0:x1] = rng.uniform(v0.min(), v0.max(), (z1 - z0, y1 - y0, x1 - x0)).astype(np.float32)
    mm1, _ = O.OracleScene(v1, colors, alphas, vr, cam, 8, 8).macrocells()
    changed = (mm0 != mm1).any(axis=-1)
    assert not (changed & ~inside).any(), np.argwhere(changed & ~inside)
    # a value above V0's range: every predicted cell sees it
    v2 = v0.copy()
    v2[z0:z1, y0:y1, x0:x1] = np.float32(v0.max() + 1.0)
    mm2, _ = O.OracleScene(v2, colors, alphas, vr, cam, 8, 8).macrocells()
    changed = (mm0 != mm2).any(axis=-1)
    assert (changed == inside).all(), (np.argwhere(changed & ~inside), np.argwhere(~changed & inside))


def test_null_handle(ovr):
    lib = ovr._lib.load()
    data = np.zeros(8, np.float32)
    lo, ext = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2)
    assert lib.ovr_hip_update_volume(None, C.c_void_p(data.ctypes.data), 0, 400, lo, ext) < 0
    assert b"null" in lib.ovr_hip_last_error()
    out = (C.c_double * 4)()
    assert lib.ovr_hip_get_update_times(None, out) < 0
    n = C.c_uint64()
    assert lib.ovr_hip_get_volume_layout(None, 0, 0, None, 0, C.byref(n)) < 0
