"""Pull-push reconstruction of sparse-sampled frames on the MI355X (include/ovr_hip.h: ovr_hip_set_reconstruction): the kernels equal
the numpy model (ovr_amd.reconstruction) bit for bit - on images of the caller and on rendered frames, with and without accumulation, in both framebuffer
sets -, sampled pixels are what the mode OFF renders, the sample lists are the CPU oracle's, and nothing changes while the mode is OFF or the frame is dense."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import make_case, oracle_scene, hip_setup, hip_frame, compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
CHECK = os.path.join(ROOT, "tests", "reconstruction_check.py")
PLUGIN = os.path.join(ROOT, "plugin", "libdevice_hip.so")
f32 = np.float32
FOCUS = ((0.5, 0.5), 0.06, 0.07)   # the benchmark's foveated configuration
COUNTERS = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "frame_index", "pipeline", "pool_chunks", "skipped_samples",
            "skipped_shadow_samples", "layout", "stale_tiles", "lds_fallback_taps", "lds_unstaged_rounds", "lds_rounds", "skipping_kernels", "tuning", "replicas_building")


def bits_differ(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def noise_tile():
    return (np.random.default_rng(11).integers(0, 256, size=(32, 32, 64)) / 255.0).astype(f32)


@pytest.fixture
def made(ovr):
    rs = []

    def make(**kw):
        r = ovr.create_renderer("hip", **kw)
        rs.append(r)
        return r

    yield make
    for r in rs:
        r.close()


def sparse_setup(ovr, ren, case, noise, mode, accumulate=False, pipeline=0, focus=FOCUS):
    ren.set_layout_choice(0)   # (a forced layout: nothing is chosen by measured times)
    hip_setup(ovr, ren, case, accumulate=accumulate, pipeline=pipeline)
    ren.set_noise_tile(noise)
    ren.set_focus(*focus)
    ren.set_sparse_sampling(True)
    ren.set_reconstruction(mode)
    ren.commit()
    return ren


def indicator(O, frame_index, w, h, noise, focus=FOCUS):
    """the ORACLE's sample list of a frame as a (H, W) 0 / 1 plane"""
    xy = O.sparse_mask(frame_index, w, h, focus[0], focus[1], focus[2], noise).reshape(-1, 2)
    m = np.zeros((h, w), f32)
    m[xy[:, 1], xy[:, 0]] = 1
    assert int(m.sum()) == len(xy)   # the list holds a pixel at most once
    return m


# ---- 1. the kernels on a caller's image: the model, bit for bit -------------------------------------------------------------------------------------

def image_case(rng, w, h, density, non_finite):
    rgba = rng.random((h, w, 4), dtype=f32)
    grad = rng.random((h, w, 3), dtype=f32) - f32(0.5)
    if density == "none":
        m = np.zeros((h, w), f32)
    elif density == "one":
        m = np.zeros((h, w), f32)
        m[rng.integers(0, h), rng.integers(0, w)] = 1
    elif density == "all":
        m = np.ones((h, w), f32)
    else:
        m = (rng.random((h, w)) < density).astype(f32) * f32(2.5)   # any positive weight means "sampled"
    if non_finite:
        for v in (np.nan, np.inf, -np.inf):
            y, x = rng.integers(0, h), rng.integers(0, w)
            rgba[y, x, rng.integers(0, 4)] = v
            y, x = rng.integers(0, h), rng.integers(0, w)
            grad[y, x, rng.integers(0, 3)] = v
    return rgba, grad, m


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (64, 64), (257, 131), (1920, 1080)])
def test_reconstruct_image_equals_the_model(ovr, made, w, h):
    import torch
    M = ovr.reconstruction
    ren = made()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(w * 7 + h)
    for density in ("none", "one", 0.02, 0.5, "all"):
        for with_grad in (True, False):
            for non_finite in (False, True):
                rgba, grad, m = image_case(rng, w, h, density, non_finite)
                if not with_grad:
                    grad = None
                exp_rgba, exp_grad = M.reconstruct(rgba, grad, m)
                t_rgba, t_m = torch.from_numpy(rgba.copy()).to(dev), torch.from_numpy(m.copy()).to(dev)
                t_grad = torch.from_numpy(grad.copy()).to(dev) if with_grad else None
                ren.reconstruct_image(t_rgba, t_grad, t_m)
                what = f"{w}x{h} density {density} grad {with_grad} non-finite {non_finite}"
                d = bits_differ(t_rgba.cpu().numpy(), exp_rgba)
                assert d == 0, f"{what}: {d} RGBA floats differ from the model"
                if with_grad:
                    d = bits_differ(t_grad.cpu().numpy(), exp_grad)
                    assert d == 0, f"{what}: {d} gradient floats differ from the model"
                assert np.array_equal(t_m.cpu().numpy(), m), f"{what}: the weight plane was modified"
                if non_finite and density not in ("none", "one"):
                    holes = m == 0
                    assert np.isfinite(t_rgba.cpu().numpy()[holes]).all(), f"{what}: a non-finite sample spread into a hole"


def test_reconstruct_image_needs_no_scene_and_checks_its_arguments(ovr, made):
    import torch
    ren = made()
    dev = torch.device("cuda", 0)
    rgba, m = torch.zeros((4, 6, 4), device=dev), torch.ones((4, 6), device=dev)
    ren.reconstruct_image(rgba, None, m)
    lib = ovr._lib.load()
    assert lib.ovr_hip_reconstruct_image(ren._h, None, None, m.data_ptr(), 6, 4) == -1
    assert lib.ovr_hip_reconstruct_image(ren._h, rgba.data_ptr(), None, m.data_ptr(), -1, 4) == -1
    assert lib.ovr_hip_set_reconstruction(ren._h, 2) == -1
    with pytest.raises(RuntimeError):
        ren.reconstruct_image(rgba, None, torch.ones((4, 5), device=dev))
    r = ren.reconstruction()
    assert r.mode == 0 and r.valid == 0 and r.levels == 0
    with pytest.raises(RuntimeError):
        ren.reconstruction_weights()   # ESTATE while the mode is OFF


# ---- 2. the render path without accumulation -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pipeline", [1, 2], ids=["in_place", "pooled"])
def test_sparse_frame_is_filled_as_the_model_says(ovr, oracle, made, pipeline):
    """both framebuffer sets (render, swap, render, ...): at the oracle's listed pixels the FILL frame is the OFF frame bit for bit and meets the parity bar
    against the oracle's sparse frame; the whole FILL frame is model(OFF frame, oracle's list); N is the list's indicator"""
    M = ovr.reconstruction
    noise = noise_tile()
    case = make_case(ovr, oracle, n=32, tf="bumps", cam="oblique", size=(100, 76), shading=2, spp=1)
    w, h = case["size"]
    sc = oracle_scene(oracle, case, sparse=True, focus=FOCUS, noise=noise)
    fill = sparse_setup(ovr, made(), case, noise, 1, pipeline=pipeline)
    off = sparse_setup(ovr, made(), case, noise, 0, pipeline=pipeline)
    for step in range(4):
        fill.render()
        off.render()
        k = fill.stats().frame_index
        assert k == off.stats().frame_index == step + 1
        m = indicator(oracle, k, w, h, noise)
        s = m > 0
        f_rgba, f_grad = hip_frame(ovr, fill)
        o_rgba, o_grad = hip_frame(ovr, off)
        assert bits_differ(f_rgba[s], o_rgba[s]) == 0 and bits_differ(f_grad[s], o_grad[s]) == 0, f"frame {k}: a sampled pixel changed"
        assert not o_rgba[~s].any() and not o_grad[~s].any()
        ref_rgba, ref_grad = np.zeros((h, w, 4), f32), np.zeros((h, w, 3), f32)
        cnt = oracle.Counters()
        sc.lib.ovr_oracle_render_frame(C.byref(sc.s), k, 0, None, oracle._fp(ref_rgba), oracle._fp(ref_grad), C.byref(cnt), 0)
        compare(oracle, np.where(s[..., None], f_rgba, 0).astype(f32), ref_rgba, name=f"frame {k}: sampled pixels against the oracle's sparse frame")
        exp_rgba, exp_grad = M.reconstruct(o_rgba, o_grad, m)
        assert bits_differ(f_rgba, exp_rgba) == 0 and bits_differ(f_grad, exp_grad) == 0, f"frame {k} (set {step & 1}): the filled frame is not the model's"
        assert bits_differ(fill.reconstruction_weights(), m) == 0
        r = fill.reconstruction()
        assert r.mode == 1 and r.valid == 1 and r.levels == len(M.levels(w, h))
        assert r.sampled_pixels == int(m.sum()) and r.filled_pixels == w * h - int(m.sum())
        assert off.reconstruction().valid == 0
        fs, os_ = fill.stats(), off.stats()
        assert {c: int(getattr(fs, c)) for c in COUNTERS} == {c: int(getattr(os_, c)) for c in COUNTERS}
        assert (f_rgba[..., 3] > 0).mean() > (o_rgba[..., 3] > 0).mean() and 0 < int(m.sum()) < w * h
        if step != 2:   # (renderbatch never swaps: one step stays in its set)
            fill.swap()
            off.swap()


# ---- 3. with accumulation -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("swap", [False, True], ids=["renderbatch_order", "swapping"])
def test_accumulated_sparse_frames(ovr, oracle, made, swap):
    """k = 1 ... 6: N is the per-pixel count of the oracle's lists; the frame is model(A / N, G / N, N) with A and G read back from the renderer; G is the sum,
    in frame order, of the gradient pixels the OFF run's frames show at the listed pixels (tests/reconstruction_check.py ties A to the oracle's buffer)"""
    M = ovr.reconstruction
    noise = noise_tile()
    case = make_case(ovr, oracle, n=32, tf="bumps", cam="oblique", size=(100, 76), shading=2, spp=1)
    w, h = case["size"]
    fill = sparse_setup(ovr, made(), case, noise, 1, accumulate=True, pipeline=2)
    off = sparse_setup(ovr, made(), case, noise, 0, accumulate=True, pipeline=2)
    N, G = np.zeros((h, w), f32), np.zeros((h, w, 3), f32)
    with pytest.raises(RuntimeError):
        fill.reconstruction_weights()   # no frame yet: no buffer
    for k in range(1, 7):
        fill.render()
        off.render()
        assert fill.stats().frame_index == k
        m = indicator(oracle, k, w, h, noise)
        s = m > 0
        N += m
        o_rgba, o_grad = hip_frame(ovr, off)
        G[s] = (G[s] + o_grad[s]).astype(f32)
        f_rgba, f_grad = hip_frame(ovr, fill)
        assert bits_differ(fill.reconstruction_weights(), N) == 0, f"frame {k}: N is not the count of the oracle's lists"
        assert bits_differ(fill.reconstruction_gradient(), G) == 0, f"frame {k}: G is not the sum of the OFF run's gradient pixels"
        A = fill.accumulation(0)
        assert bits_differ(A, off.accumulation(0)) == 0
        exp_rgba, exp_grad = M.reconstruct(*M.level0(A, G, N), N)
        assert bits_differ(f_rgba, exp_rgba) == 0 and bits_differ(f_grad, exp_grad) == 0, f"frame {k}: the filled frame is not the model's"
        r = fill.reconstruction()
        assert r.valid == 1 and r.sampled_pixels == int((N > 0).sum())
        # a sampled pixel shows A / N, not the OFF run's A / n (dimmed by N / n)
        assert bits_differ(f_rgba[N > 0], (A[N > 0] / N[N > 0][:, None]).astype(f32)) == 0
        if swap:
            fill.swap()
            off.swap()
    assert N.max() >= 2 and (N == 0).any()


def test_exact_against_the_oracle_on_the_parity_instrument():
    """tests/reconstruction_check.py on libovr_hip_parity.so: A is the oracle's accumulation buffer, so the chain frame == model(A / N, G / N, N) ends at the oracle"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_ORACLE_POWF="det")
    env.pop("OVR_HIP_POOL_CHUNKS", None)
    out = subprocess.run([sys.executable, CHECK, "exact"], env=env, capture_output=True, text=True, timeout=900)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "all exact" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_pool_overflow_counts_the_frame_once(tmp_path):
    """OVR_HIP_POOL_CHUNKS=8 (the existing diagnostic) makes an early pooled frame overflow the request pool: it is rendered again, and N, G, A and the frames
    are those of a run without the overflow (the overflowing attempt wrote no pixel, counted nothing and filled nothing)"""
    outs = []
    for k, chunks in enumerate((None, "8")):
        env = dict(os.environ)
        env.pop("OVR_HIP_POOL_CHUNKS", None)
        if chunks:
            env["OVR_HIP_POOL_CHUNKS"] = chunks
        path = str(tmp_path / f"run{k}.npz")
        out = subprocess.run([sys.executable, CHECK, "overflow", path], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        outs.append(np.load(path))
    a, b = outs
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 6 * 6
    for k in a.files:
        if k.startswith("chunks"):
            assert a[k][0] > 0 and b[k][0] > 0   # both ran the pooled pipeline
            continue
        assert bits_differ(a[k], b[k]) == 0, k
    assert a["N6"].max() >= 2 and np.array_equal(a["N1"], (a["N1"] > 0).astype(f32))


# ---- 4. mapping, quality, states --------------------------------------------------------------------------------------------------------------------------

def test_host_mapping_covers_the_whole_filled_frame(ovr, oracle, made):
    """a camera whose box covers a small part of the image: mapframe(HOST) copies only the box's rectangle of an ordinary frame - a filled frame is not 0
    outside it and is mapped whole: the host copy equals the device frame on every pixel, in both sets"""
    noise = noise_tile()
    case = make_case(ovr, oracle, n=24, tf="dense", cam="oblique", size=(160, 120), shading=2, spp=1, fovy=100.0)
    dense = hip_setup(ovr, made(), case)
    dense.render()
    ys, xs = np.nonzero(hip_frame(ovr, dense)[0][..., 3])
    x0, x1, y0, y1 = xs.min(), xs.max(), ys.min(), ys.max()
    assert (x1 - x0 + 1) * (y1 - y0 + 1) < 0.5 * 160 * 120   # the box's silhouette is a small part of the image
    ren = sparse_setup(ovr, made(), case, noise, 1)
    outside = np.ones((120, 160), bool)
    outside[y0:y1 + 1, x0:x1 + 1] = False
    bled = 0
    for step in range(4):
        ren.render()
        host_rgba, host_grad = hip_frame(ovr, ren)
        fb = ovr.FrameBufferData()
        ren.mapframe(fb, device=True)
        dev_rgba, dev_grad = fb.rgba.data().cpu().numpy(), fb.grad.data().cpu().numpy()
        assert bits_differ(host_rgba, dev_rgba) == 0 and bits_differ(host_grad, dev_grad) == 0, f"frame {step + 1}: the host copy is not the device frame"
        bled += int((dev_rgba[..., 3][outside] != 0).sum())
        ren.swap()
    assert bled > 0   # the interpolation does reach pixels outside the silhouette's bounding box


def test_filling_brings_the_frame_closer_to_the_dense_one(ovr, oracle, made):
    """a condition, not a number: the mean absolute RGBA error against the oracle's DENSE frame is smaller with the holes filled than with the holes left"""
    noise = noise_tile()
    case = make_case(ovr, oracle, n=32, tf="bumps", cam="oblique", size=(256, 256), shading=2, spp=1)
    dense = oracle_scene(oracle, case).render(frames=1)[0]
    frames = {}
    for mode in (0, 1):
        ren = sparse_setup(ovr, made(), case, noise, mode)
        ren.render()
        frames[mode] = hip_frame(ovr, ren)[0]
    err = {mode: float(np.abs(frames[mode].astype(np.float64) - dense).mean()) for mode in (0, 1)}
    psnr = {mode: float(10 * np.log10(1.0 / max(np.mean((frames[mode].astype(np.float64) - dense) ** 2), 1e-30))) for mode in (0, 1)}
    print(f"quality 256x256, focus {FOCUS}: mean |error| OFF {err[0]:.6f} FILL {err[1]:.6f}; PSNR OFF {psnr[0]:.2f} dB FILL {psnr[1]:.2f} dB; "
          f"sampled {(frames[0][..., 3] > 0).mean() * 100:.1f} % of the pixels have alpha")
    assert err[1] < err[0]


def test_group_handles_refuse_and_image_shards_are_left_alone(ovr, oracle, made):
    noise = noise_tile()
    case = make_case(ovr, oracle, n=32, tf="bumps", cam="oblique", size=(100, 76), shading=2, spp=1)
    group = made(devices=[0, 0])
    lib = ovr._lib.load()
    assert lib.ovr_hip_set_reconstruction(group._h, 1) == -3   # OVR_HIP_ESTATE
    assert b"device group" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_set_reconstruction(group._h, 0) == 0
    got = []
    for mode in (0, 1):
        ren = made()
        ren.set_layout_choice(0)
        hip_setup(ovr, ren, case)
        ren.set_noise_tile(noise)
        ren.set_focus(*FOCUS)
        ren.set_sparse_sampling(True)
        ren.set_image_shard(1, 3, 16, 16)
        ren.set_reconstruction(mode)
        ren.commit()
        ren.render()
        got.append(hip_frame(ovr, ren))
        r = ren.reconstruction()
        assert r.mode == mode and r.valid == 0
    assert bits_differ(got[0][0], got[1][0]) == 0 and bits_differ(got[0][1], got[1][1]) == 0


def test_modes_and_resets(ovr, oracle, made):
    """OFF after FILL frees the buffers and gives the frames of a renderer on which the mode was never set (`fresh`: the same calls, the same resets - made with
    another setter -, never ovr_hip_set_reconstruction); a dense frame under FILL is the OFF frame with equal counters; sparse sampling off and on again, and
    the setter itself, restart N"""
    noise = noise_tile()
    case = make_case(ovr, oracle, n=32, tf="bumps", cam="oblique", size=(100, 76), shading=2, spp=1)
    w, h = case["size"]

    def snapshot(ren):
        ren.render()
        st = ren.stats()
        return hip_frame(ovr, ren) + ({c: int(getattr(st, c)) for c in COUNTERS},)

    for accumulate in (False, True):
        ren = sparse_setup(ovr, made(), case, noise, 1, accumulate=accumulate, pipeline=2)
        fresh = made()
        fresh.set_layout_choice(0)
        hip_setup(ovr, fresh, case, accumulate=accumulate, pipeline=2)
        fresh.set_noise_tile(noise)
        fresh.set_focus(*FOCUS)
        fresh.set_sparse_sampling(True)
        fresh.commit()
        pair = (ren, fresh)
        for _ in range(3):
            for r in pair:
                r.render()
                r.swap()
        assert ren.reconstruction().valid == 1 and fresh.reconstruction().valid == 0
        # the setter resets the accumulation (fresh: any other setter does)
        ren.set_reconstruction(1)
        fresh.set_focus(*FOCUS)
        for r in pair:
            r.commit()
            r.render()
        k = ren.stats().frame_index
        assert k == fresh.stats().frame_index and (k == 1 if accumulate else k == 4)
        assert bits_differ(ren.reconstruction_weights(), indicator(oracle, k, w, h, noise)) == 0
        # sparse sampling off: dense frames under FILL are the OFF frames, with the same counters
        for r in pair:
            r.set_sparse_sampling(False)
            r.commit()
        for _ in range(2):
            a, b = snapshot(ren), snapshot(fresh)
            assert bits_differ(a[0], b[0]) == 0 and bits_differ(a[1], b[1]) == 0 and a[2] == b[2]
            assert ren.reconstruction().valid == 0 and ren.reconstruction().mode == 1
            for r in pair:
                r.swap()
        # ... and on again: no stale N
        for r in pair:
            r.set_sparse_sampling(True)
            r.commit()
            r.render()
        k = ren.stats().frame_index
        assert bits_differ(ren.reconstruction_weights(), indicator(oracle, k, w, h, noise)) == 0
        # OFF: the buffers go, the frames are the fresh renderer's
        ren.set_reconstruction(0)
        fresh.set_focus(*FOCUS)
        for r in pair:
            r.commit()
        for _ in range(3):
            a, b = snapshot(ren), snapshot(fresh)
            assert bits_differ(a[0], b[0]) == 0 and bits_differ(a[1], b[1]) == 0 and a[2] == b[2]
            assert not a[0][indicator(oracle, a[2]["frame_index"], w, h, noise) == 0].any() or accumulate   # holes again
            for r in pair:
                r.swap()
        with pytest.raises(RuntimeError):
            ren.reconstruction_weights()
        assert ren.reconstruction().mode == 0 and ren.reconstruction().valid == 0


# ---- 5. the plugin ------------------------------------------------------------------------------------------------------------------------------------------

def test_plugin_variable(tmp_path, ovr, made):
    """oracle/_ref/plugin_probe renders three accumulated sparse frames through the reference's MainRenderer interface: with OVR_HIP_RECONSTRUCT=1 its frame is
    the Python host's with the mode on (to the few ulp by which the two hosts rasterise the transfer function, as tests/test_renderbatch_gpu.py allows), without
    the variable it is the frame with holes"""
    probe = os.path.join(ROOT, "oracle", "_ref", "plugin_probe")
    if not (os.path.exists(probe) and os.path.exists(PLUGIN)):
        pytest.skip("oracle/_ref/plugin_probe or plugin/libdevice_hip.so missing (built by __graft_entry__.build() where the reference tree is present)")
    n, W, H = 40, 112, 72
    vol = ovr.synth.make_volume(n, np.float32)
    colors, alphas, vr = ovr.synth.make_tfn("bumps", 256)
    cam = ovr.synth.make_camera("oblique", n)
    scene_path = ovr.vidi3d.write_scene(str(tmp_path), "synthetic", vol, ovr.synth._RAINBOW, alphas[1::2].copy(), (0.0, 1.0), cam, fovy=45.0, sample_distance=0.5)
    tile = np.random.default_rng(7).random((32, 32, 64), dtype=np.float32)
    tile.tofile(str(tmp_path / "noise.bin"))
    got = {}
    for mode in (0, 1):
        env = dict(os.environ)
        env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.dirname(PLUGIN), os.path.join(ROOT, "open-volume-renderer_amd"), env.get("LD_LIBRARY_PATH", "")])
        env["OVR_HIP_NOISE_TILE"] = str(tmp_path / "noise.bin")
        env.pop("OVR_HIP_RECONSTRUCT", None)
        env.pop("OVR_HIP_QUIET", None)
        if mode:
            env["OVR_HIP_RECONSTRUCT"] = "1"
        out = subprocess.run([probe, scene_path, str(W), str(H), str(tmp_path / f"frames{mode}.f32")], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert ("[hip] reconstruction of sparse-sampled frames: on" in out.stderr) == bool(mode)
        got[mode] = np.fromfile(str(tmp_path / f"frames{mode}.f32"), dtype=np.float32).reshape(2, H, W, 4)
    scene, camera = ovr.vidi3d.scene_from_file(scene_path)
    mine = {}
    for mode in (0, 1):
        ren = made()
        ren.set_fbsize((W, H))
        ren.set_frame_accumulation(True)
        ren.set_sample_per_pixel(2)
        ren.set_volume_sampling_rate(scene.volume_sampling_rate)
        ren.set_noise_tile(tile)
        ren.init(scene, camera)
        ren.set_reconstruction(mode)
        ren.commit()
        ren.set_sparse_sampling(True)
        ren.set_focus((0.4, 0.6), 0.3, 0.05)
        ren.commit()
        for _ in range(3):
            ren.render()
        mine[mode] = hip_frame(ovr, ren)[0]
    for mode in (0, 1):
        assert np.abs(got[mode][0] - mine[mode]).max() <= 2e-5, mode
    assert np.abs(got[0][1] - got[1][1]).max() == 0   # the dense frames behind it do not depend on the mode
    assert (got[1][0][..., 3] > 0).mean() > (got[0][0][..., 3] > 0).mean()
