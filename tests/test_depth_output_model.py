"""The depth-layer model (open-volume-renderer_amd/depth_output.py, include/ovr_hip.h ovr_hip_set_depth_output) on the CPU: its picture and counters are
max_depth.rays' under an all-+inf image bit for bit (and through tests/test_max_depth_model.py the unmodified oracle's march); its depth d, handed back as a
depth limit, makes the limited march take exactly k steps; over a constant volume k is the closed form of the float recurrence; a limit in front of the crossing
leaves nothing reached.  Then the helpers (planar_from_ray_distance, resolve, check, active) and the inputs of the GPU comparison: few borderline rays.  No GPU."""
import os
import re

import numpy as np
import pytest

import depth_output_cases as DC
import max_depth_cases as MC
import preintegration_cases as QC
import projection_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ["ovr_hip_set_depth_output", "ovr_hip_get_depth_output", "ovr_hip_depth_output_floats"]
_cache = {}


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _axis_rays(ovr, oracle):
    basis = oracle.camera_basis(*PC.CAMERAS[DC.CAMERA], PC.FOVY, *DC.SIZE).reshape(4, 3)
    d = ovr.projection.pixel_rays(basis, *DC.SIZE).reshape(-1, 3)
    return basis, np.broadcast_to(np.asarray(basis[0], F), d.shape), d


def _committed(ovr, oracle, dtype, tau):
    """the committed case's rays under tau, and the unlimited max_depth.rays beside them (computed once per type)"""
    name = np.dtype(dtype).name
    vol = QC.volume(DC.VOLUME, dtype)
    _, ct, at, tfr = MC.case_tables(ovr, dtype)
    basis, org, d = _axis_rays(ovr, oracle)
    if ("march", name) not in _cache:
        _cache[("march", name)] = ovr.max_depth.rays(vol, org, d, np.full(len(org), np.inf, F), DC.RATE, ct, at, tfr, border=DC.BORDER)
    if ("depth", name, tau) not in _cache:
        _cache[("depth", name, tau)] = ovr.depth_output.rays(vol, org, d, tau, DC.RATE, ct, at, tfr, border=DC.BORDER)
    return vol, (ct, at, tfr), org, d, _cache[("march", name)], _cache[("depth", name, tau)]


# ---- entry points and header ------------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_bound_and_exported(ovr):
    hdr = open(os.path.join(ROOT, "include", "ovr_hip.h")).read()
    lib = ovr._lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in ovr._lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define OVR_HIP_DEPTH_OUTPUT_OFF 0\b", hdr) and re.search(r"#define OVR_HIP_DEPTH_OUTPUT_ON 1\b", hdr)
    assert (ovr._lib.DEPTH_OUTPUT_OFF, ovr._lib.DEPTH_OUTPUT_ON) == (0, 1)
    assert lib.ovr_hip_abi_version() == 11
    assert lib.ovr_hip_set_depth_output(None, 0, 0.0) < 0 and lib.ovr_hip_get_depth_output(None, None) < 0
    assert lib.ovr_hip_depth_output_floats(None, None, None, None, None, 0, 0, 0.5) < 0
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 27." in design and "Not done" in design.split("## 27.")[1]
    assert "ovr_hip_set_depth_output" in open(os.path.join(ROOT, "README.md")).read()
    assert "OVR_HIP_DEPTH_OUTPUT_FILE" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("set_depth_output", "get_depth_output", "depth_output_rays"):
        assert hasattr(ovr.DeviceHIP, name), name
    for name in ("check", "active", "rays", "frame", "resolve", "planar_from_ray_distance"):
        assert hasattr(ovr.depth_output, name), name


# ---- the frame identity: the picture is the march's ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tau", DC.TAUS, ids=lambda t: "tau=%g" % t)
@pytest.mark.parametrize("dtype", (np.float32, np.uint8), ids=("f32", "u8"))
def test_the_picture_and_the_counters_are_the_marchs(ovr, oracle, dtype, tau):
    _, _, _, _, march, depth = _committed(ovr, oracle, dtype, tau)
    assert _same(depth["rgba"], march["rgba"])
    for key in ("steps", "shaded", "rays_hit", "borderline", "hinge", "borderline_steps"):
        assert np.array_equal(depth[key], march[key]), key
    assert _same(depth["tc"], march["tc"]) and _same(depth["tx"], march["tx"])
    assert march["steps"].sum() > 1500 and march["shaded"].sum() > 1000


@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
def test_a_depth_frame_is_the_depth_limited_frame(ovr, oracle, shading):
    """as frames, with the committed plane and without an image, shaded and not: rgba and counters are max_depth.frame's"""
    vol = QC.volume(DC.VOLUME, np.float32)
    _, ct, at, tfr = MC.case_tables(ovr, np.float32)
    basis = oracle.camera_basis(*PC.CAMERAS[DC.CAMERA], PC.FOVY, *DC.SIZE).reshape(4, 3)
    for image in (None, MC.plane_image()):
        limit = np.full(DC.SIZE[::-1], np.inf, F) if image is None else image
        want = ovr.max_depth.frame(vol, basis, DC.SIZE, limit, DC.RATE, ct, at, tfr, shading=shading, light=DC.LIGHT, intensity=DC.INTENSITY, material=DC.MATERIAL)
        got = ovr.depth_output.frame(vol, basis, DC.SIZE, 0.5, DC.RATE, ct, at, tfr, depth=image, shading=shading, light=DC.LIGHT, intensity=DC.INTENSITY, material=DC.MATERIAL)
        assert _same(got[0], want[0]) and all(got[2][k] == want[2][k] for k in ("rays", "rays_hit", "samples", "shaded", "hinge", "borderline_steps"))
        assert got[1][..., 2].any() and set(np.unique(got[1][..., 2])) <= {0.0, 1.0}


# ---- the round trip: d handed back as a depth limit ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tau", DC.TAUS, ids=lambda t: "tau=%g" % t)
@pytest.mark.parametrize("dtype", (np.float32, np.uint8), ids=("f32", "u8"))
def test_the_depth_handed_back_as_a_limit_takes_exactly_k_steps(ovr, oracle, dtype, tau):
    vol, (ct, at, tfr), org, d, march, depth = _committed(ovr, oracle, dtype, tau)
    reached, hit = depth["reached"], depth["rays_hit"]
    z = np.where(reached, depth["d"], F(np.inf)).astype(F)
    lim = ovr.max_depth.rays(vol, org, d, z, DC.RATE, ct, at, tfr, border=DC.BORDER)
    a_full, a_lim = march["rgba"][:, 3], lim["rgba"][:, 3]
    assert np.array_equal(lim["steps"][reached], depth["k"][reached]) and (depth["k"][reached] >= 1).all() and not depth["k"][~reached].any() and not depth["d"][~reached].any()
    assert _same(lim["tx"][reached], depth["d"][reached])
    assert (a_lim[reached] >= F(tau)).all() and (a_lim[reached] <= a_full[reached]).all()
    assert _same(lim["rgba"][~reached], march["rgba"][~reached]) and np.array_equal(lim["steps"][~reached], march["steps"][~reached])
    # S / alpha is a depth inside the ray's interval
    lit = a_full > 0
    mean = depth["S"][lit].astype(np.float64) / a_full[lit].astype(np.float64)
    slack = 1e-5 * depth["t1"][lit].astype(np.float64)      # (S and alpha are float32 sums of up to 40 terms)
    assert (mean >= depth["t0"][lit] - slack).all() and (mean <= depth["t1"][lit] + slack).all() and not depth["S"][~lit].any()
    # not degenerate: reached, lit without reaching (but at the smallest tau, where lit is reached), saturated
    saturated = a_full >= 0.9999
    print(np.dtype(dtype).name, tau, "hit", int(hit.sum()), "lit", int(lit.sum()), "reached", int(reached.sum()), "saturated", int(saturated.sum()),
          "near 0.9999", int(depth["borderline"].sum()), "near tau", int(depth["near_tau"].sum()))
    assert hit.sum() > 500 and reached.sum() > 300 and saturated.sum() > 30 and (~reached & ~hit).sum() > 100
    if tau == DC.TAU_FIRST:
        assert np.array_equal(reached, lit)
        first = depth["k"][reached]
        assert (first >= 1).all() and (first < march["steps"][reached]).any()
    else:
        assert (lit & ~reached).sum() > 20 and (depth["k"][reached] < march["steps"][reached]).sum() > 100
    if dtype is np.float32:      # the counts the issue's prototype gave for this case
        assert hit.sum() == 572 and {0.25: 500, 0.5: 480, 0.9: 377}.get(tau, int(reached.sum())) == reached.sum(), (int(hit.sum()), int(reached.sum()))


# ---- the closed form over a constant volume ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tau", (DC.TAU_FIRST, 0.25, 0.5, 0.9))
def test_over_a_constant_volume_k_is_the_recurrences_first_crossing(ovr, tau):
    _, colors, alphas, vr = DC.ramp_volume_and_tables(ovr)
    ct, at = PC.tables(colors, alphas)
    vol = DC.constant_volume(0.5 * (vr[0] + vr[1]))
    org, d = DC.dyadic_rays()
    r = ovr.depth_output.rays(vol, org, d, tau, 1.0, ct, at, vr)
    assert r["rays_hit"].all()
    # the one corrected opacity of a whole step (dt = 1 exactly on these rays), by the model's own pieces
    a_tf = ovr.projection.classify(np.array([vol[0, 0, 0]], F), ct, at, *vr)[0, 3]
    a = ovr.slice_context.opacity_correction(np.array([a_tf], F), ovr.max_depth.BASE, np.array([1], F))[0]
    assert 0 < a < 0.6
    alpha, seq = F(0), []
    while alpha < F(0.9999) and len(seq) < 64:      # the march's float recurrence, alpha = fma(1 - alpha, a, alpha)
        alpha = F(ovr.lighting.fma(np.array([F(1) - alpha], F), np.array([a], F), np.array([alpha], F))[0])
        seq.append(alpha)
    k_want = next((i + 1 for i, v in enumerate(seq) if v >= F(tau)), None)
    whole = np.floor((r["t1"] - r["t0"]).astype(np.float64)).astype(np.int64)      # the steps of length exactly 1
    if k_want is None:
        assert not r["reached"][whole < 64].any()
        return
    can = whole >= k_want
    assert can.sum() > 20, (k_want, int(can.sum()))
    assert (r["k"][can] == k_want).all() and r["reached"][can].all(), (k_want, r["k"][can])
    assert _same(r["d"][can], (r["t0"][can] + F(k_want)).astype(F)) and ((r["t0"][can].astype(np.float64) + k_want) == r["d"][can].astype(np.float64)).all()
    assert not r["reached"][whole < k_want - 1].any()


# ---- a limit in front of the crossing ---------------------------------------------------------------------------------------------------------------------------------

def test_a_depth_limit_in_front_of_the_crossing_leaves_nothing_reached(ovr, oracle):
    vol, (ct, at, tfr), org, d, march, depth = _committed(ovr, oracle, np.float32, 0.5)
    reached = depth["reached"]
    later = reached & (depth["k"] >= 2)
    assert later.sum() > 100
    # one step in front of the crossing step's back end: the limited march stops k - 1 steps in
    z = np.where(later, (depth["d"] - F(1) / F(DC.RATE)).astype(F), F(np.inf)).astype(F)
    cut = ovr.depth_output.rays(vol, org, d, 0.5, DC.RATE, ct, at, tfr, depth=z)
    assert not cut["reached"][later].any() and not cut["d"][later].any() and not cut["k"][later].any() and (cut["layer"][later][:, [0, 2]] == 0).all()
    assert (cut["rgba"][later, 3] < F(0.5)).all() and (cut["S"][later] > 0).sum() > 50
    others = ~later
    assert np.array_equal(cut["reached"][others], depth["reached"][others]) and _same(cut["d"][others], depth["d"][others]) and _same(cut["S"][others], depth["S"][others])
    # and against max_depth.rays under the same depths: the picture is the depth-limited one
    lim = ovr.max_depth.rays(vol, org, d, z, DC.RATE, ct, at, tfr)
    assert _same(cut["rgba"], lim["rgba"]) and np.array_equal(cut["steps"], lim["steps"])


# ---- helpers -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_planar_from_ray_distance_inverts_ray_distance_from_planar(ovr, oracle):
    D, M = ovr.depth_output, ovr.max_depth
    size = (37, 23)
    rng = np.random.default_rng(27)
    z = (30.0 + 40.0 * rng.random(size[::-1])).astype(F)
    z[0, 0] = np.inf
    persp = oracle.camera_basis(*PC.CAMERAS["oblique"], PC.FOVY, *size).reshape(4, 3)
    ortho = ovr.camera.basis(*PC.CAMERAS["oblique"], *size, orthographic_height=MC.ORTHO_HEIGHT)
    for basis, kind in ((persp, 0), (ortho, ovr.camera.ORTHOGRAPHIC)):
        t = M.ray_distance_from_planar(basis, size, z, kind)
        back = D.planar_from_ray_distance(basis, size, t, kind)
        assert back.dtype == F and back.shape == z.shape and np.isinf(back[0, 0])
        fin = np.isfinite(z)
        assert np.abs(back[fin].astype(np.float64) / z[fin] - 1).max() <= 2 ** -22, kind      # two float32 roundings
        if kind:
            assert _same(back, z)
        else:
            assert (t[fin] >= z[fin]).all() and (t[fin] > z[fin] * 1.01).any()


def test_resolve_gives_inf_where_a_depth_is_undefined(ovr):
    rgba = np.array([[[0.1, 0.2, 0.3, 0.5], [0, 0, 0, 0], [0.1, 0.2, 0.3, 0.25], [0.5, 0.5, 0.5, 1.0]]], F)
    layer = np.array([[[61.0, 31.0, 1.0], [0, 0, 0], [0.0, 16.0, 0.0], [20.0, 65.0, 1.0 / 3.0]]], F)
    thr, mean, share = ovr.depth_output.resolve(rgba, layer)
    assert thr.dtype == F and thr.shape == (1, 4)
    assert _same(thr, np.array([[61.0, np.inf, np.inf, F(20.0) / F(1.0 / 3.0)]], F))
    assert _same(mean, np.array([[62.0, np.inf, 64.0, 65.0]], F))
    assert _same(share, layer[..., 2])
    assert ovr.max_depth.check(thr, 4, 1).shape == (1, 4)      # an output is an image the depth limit takes


def test_check_refuses_what_the_setter_refuses_and_active_is_the_rule(ovr):
    D = ovr.depth_output
    assert D.check(D.OFF, float("nan")) == (0, F(0)) and D.check(D.ON, 0.5) == (1, F(0.5)) and D.check(D.ON, D.TAU_FIRST)[1] == np.finfo(F).tiny
    assert D.check(D.ON, 0.9999)[1] == F(0.9999)
    for mode, t in ((2, 0.5), (-1, 0.5), (D.ON, 0.0), (D.ON, -0.5), (D.ON, float("nan")), (D.ON, float(np.nextafter(F(0.9999), F(1)))), (D.ON, 1.0), (D.ON, float("inf"))):
        with pytest.raises(ValueError):
            D.check(mode, t)
    assert D.active(D.ON) and D.active(D.ON, shading=1) and not D.active(D.OFF) and not D.active(D.ON, shading=2)
    assert not D.active(D.ON, slices=1) and not D.active(D.ON, isovalues=2) and not D.active(D.ON, projection_mode=1)
    assert not D.active(D.ON, preintegration=1) and D.active(D.ON, shading=1, preintegration=1)
    assert not D.active(D.ON, gradient_opacity_mode=1) and not D.active(D.ON, shading=1, gradient_opacity_mode=1)
    assert D.limited(D.ON, True, (4, 3), (4, 3)) and not D.limited(D.ON, True, (4, 3), (3, 4)) and not D.limited(D.ON, False, (4, 3), (4, 3)) and not D.limited(D.OFF, True, (4, 3), (4, 3))


# ---- the inputs of the GPU comparison stay under the borderline cap ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tau", DC.GPU_TAUS, ids=lambda t: "tau=%g" % t)
@pytest.mark.parametrize("dtype", QC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_committed_case_and_the_seeded_rays_have_few_borderline_rays(ovr, oracle, dtype, tau):
    D = ovr.depth_output
    vol = QC.volume(DC.VOLUME, dtype)
    _, ct, at, tfr = MC.case_tables(ovr, dtype)
    basis, org, d = _axis_rays(ovr, oracle)
    sorg, sd, sz = DC.seeded_rays()
    for shading in (0, 1):
        sets = (("committed", org, d, None), ("committed, plane", org, d, MC.plane_image().reshape(-1)), ("seeded, short chords", *DC.short_chord_rays(ovr), None), ("seeded, depths", sorg, sd, sz))
        for name, o, dd, z in sets:
            r = D.rays(vol, o, dd, tau, DC.RATE, ct, at, tfr, depth=z, shading=shading, light=DC.LIGHT, intensity=DC.INTENSITY, material=DC.MATERIAL, cam_pos=basis[0], border=DC.BORDER)
            b, hit = D.borderline_rays(r, tau), r["rays_hit"]
            print(np.dtype(dtype).name, tau, shading, name, "hit", int(hit.sum()), "reached", int(r["reached"].sum()), "borderline", int(b.sum()), "of them near tau", int(r["near_tau"].sum()))
            assert b.sum() <= DC.BORDER_CAP * hit.sum(), (name, int(b.sum()), int(hit.sum()))
            assert r["reached"].sum() > 100, name
    whole = D.rays(vol, sorg, sd, tau, DC.RATE, ct, at, tfr, border=DC.BORDER)      # why the run without depths takes the short chords: the whole set is over the cap
    print(np.dtype(dtype).name, tau, "all seeded rays without depths: borderline", int(D.borderline_rays(whole, tau).sum()), "of", int(whole["rays_hit"].sum()))


@pytest.mark.parametrize("tau", DC.GPU_TAUS, ids=lambda t: "tau=%g" % t)
@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
def test_the_jittered_frames_have_few_borderline_pixels(ovr, oracle, shading, tau):
    vol = QC.volume(DC.VOLUME, np.float32)
    _, ct, at, tfr = MC.case_tables(ovr, np.float32)
    basis = oracle.camera_basis(*PC.CAMERAS[DC.CAMERA], PC.FOVY, *DC.SIZE).reshape(4, 3)
    noise = DC.noise_tile()
    marked, hit_rays = np.zeros(DC.SIZE[::-1], bool), 0
    for frame_index in (1, 2):
        c = ovr.depth_output.frame(vol, basis, DC.SIZE, tau, DC.RATE, ct, at, tfr, shading=shading, light=DC.LIGHT, intensity=DC.INTENSITY, material=DC.MATERIAL, spp=3, noise=noise,
                                   frame_index=frame_index)[2]
        marked |= c["borderline"]
        hit_rays += c["rays_hit"]
    print("shading", shading, "tau", tau, "borderline pixels", int(marked.sum()), "hit rays", hit_rays)
    assert hit_rays > 3000 and marked.sum() <= DC.BORDER_CAP * hit_rays, (int(marked.sum()), hit_rays)
