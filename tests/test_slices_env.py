"""OVR_HIP_SLICES as the plugin parses it (plugin/slices_env.hpp), the host arithmetic of ovr_hip_set_slices (csrc/host/slices_host.hpp) - both through a
stand-alone program built with the address and undefined-behaviour sanitizers - and the scene file's `view.volume.slice` block as vidi3d reads and writes it.
No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("slices_host") / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", HOST, "-I", os.path.join(ROOT, "plugin"),
                           os.path.join(ROOT, "tests", "slices_host_driver.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("scenario", ("host_values", "env_parser"))
def test_host_arithmetic_and_parser_under_sanitizers(driver, scenario):
    p = subprocess.run([driver, scenario], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr


def test_the_plugin_and_the_setter_use_them():
    assert "ovrhip_plugin::parse_slices(sv" in open(os.path.join(ROOT, "plugin", "device_hip.cpp")).read()
    assert "slice_values(slices[k].point" in open(os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "ovr_hip_api.cpp")).read()


def test_the_model_and_the_host_header_agree(ovr, driver):
    """slices.commit is the same arithmetic in numpy: the literals the driver holds the header to"""
    c = ovr.slices.commit([((20.0, 16.5, 9.0), (1.0, 2.0, -1.0), 3.0, 3)])[0]
    assert [float(x).hex() for x in c["n"]] == ["0x1.a20bd80000000p-2", "0x1.a20bd80000000p-1", "-0x1.a20bd80000000p-2"]
    assert c["c"] == np.float32((c["n"].astype(np.float64) * (20.0, 16.5, 9.0)).sum())


def _write(ovr, tmp_path, name, dims, slices, spacing=None, clipping_box=None):
    nx, ny, nz = dims
    vol = np.zeros((nz, ny, nx), np.uint8)
    path = ovr.vidi3d.write_scene(str(tmp_path), name, vol, [(0.0, 0, 0, 0), (1.0, 1, 1, 1)], np.linspace(0, 1, 16).astype(np.float32), (0.0, 1.0),
                                  ((0, 0, -50), (0, 0, 0), (0, 1, 0)), slices=slices, clipping_box=clipping_box)
    if spacing is not None:   # (the writer has no spacing argument: the data source's `scales`, as the shipped scenes with one carry it)
        import json
        doc = json.load(open(path))
        doc["dataSource"][0]["scales"] = dict(zip("xyz", spacing))
        json.dump(doc, open(path, "w"), indent=1)
    return path


def test_scene_file_slices_round_trip(ovr, tmp_path):
    dims = (40, 33, 18)
    p = _write(ovr, tmp_path, "a", dims, {"x": (10.0, True), "y": (16.5, False), "z": (4.5, True)})
    d = ovr.vidi3d.read_scene(p, load_volume=False)
    assert [s["normal"] for s in d["slices"]] == [(1.0, 0.0, 0.0), (0.0, 0.0, 1.0)]          # the visible ones, in the order x, y, z
    assert all(s["thickness"] == 0.0 and s["mode"] == 1 for s in d["slices"])
    assert np.allclose(d["slices"][0]["point"], (10.0, 16.5, 9.0), atol=1e-12) and np.allclose(d["slices"][1]["point"], (20.0, 16.5, 4.5), atol=1e-12)
    assert d["clipping_box"] is None          # a bounding box written for the slices alone is no clipping box
    # the file holds the position in the bounding box's units, (0 .. dims - 1), as the clipping box's
    import json
    jv = json.load(open(p))["view"]["volume"]
    assert jv["slice"]["x"] == {"position": 10.0 / 40 * 39, "visible": True} and jv["slice"]["y"]["visible"] is False and jv["boundingBox"]["maximum"] == {"x": 39.0, "y": 32.0, "z": 17.0}
    # the values the setter takes: what the model commits from them
    c = ovr.slices.commit(d["slices"])
    assert c[0]["c"] == np.float32(d["slices"][0]["point"][0]) and c[1]["c"] == np.float32(d["slices"][1]["point"][2]) and all(s["half"] == 0 for s in c)
    # none visible, and no block at all: an empty list; the file without slices is the file it was
    q = _write(ovr, tmp_path, "b", dims, {"x": (10.0, False), "y": (1.0, False), "z": (2.0, False)})
    assert ovr.vidi3d.read_scene(q, load_volume=False)["slices"] == []
    r = _write(ovr, tmp_path, "c", dims, None)
    assert ovr.vidi3d.read_scene(r, load_volume=False)["slices"] == [] and '"slice"' not in open(r).read() and "boundingBox" not in open(r).read()
    # next to a clipping box: both are mapped the same way
    lower, upper = (4.0, 0.0, 2.0), (30.0, 33.0, 18.0)
    s = _write(ovr, tmp_path, "d", dims, {"z": (6.25, True)}, clipping_box=(lower, upper))
    d = ovr.vidi3d.read_scene(s, load_volume=False)
    assert np.allclose(d["clipping_box"][0], lower) and np.allclose(d["clipping_box"][1], upper) and np.allclose(d["slices"][0]["point"], (20.0, 16.5, 6.25))
    scene, _ = ovr.vidi3d.scene_from_file(_write(ovr, tmp_path, "e", dims, {"y": (8.0, True)}))
    assert len(scene.slices) == 1 and scene.slices[0]["normal"] == (0.0, 1.0, 0.0)


def test_scene_file_slices_with_a_spacing(ovr, tmp_path):
    dims, spacing = (24, 20, 17), (0.5, 2.0, 1.25)
    p = _write(ovr, tmp_path, "s", dims, {"x": (6.0, True), "z": (17.0, True)}, spacing=spacing)
    d = ovr.vidi3d.read_scene(p, load_volume=False)
    # the writer's positions are fractions of the voxel box; the world box is spacing * dims: x 6 / 24 of 12 world units, z 17 / 17 of 21.25
    assert np.allclose(d["slices"][0]["point"], (3.0, 20.0, 10.625)) and np.allclose(d["slices"][1]["point"], (6.0, 20.0, 21.25)) and d["grid_spacing"] == spacing


def test_shipped_scenes_have_no_visible_slice(ovr):
    names = sorted(n for n in os.listdir(SCENES) if n.startswith("scene_") and n.endswith(".json"))
    assert len(names) > 10
    for n in names:
        assert ovr.vidi3d.read_scene(os.path.join(SCENES, n), load_volume=False)["slices"] == [], n
