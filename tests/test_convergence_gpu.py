"""The convergence estimate and adaptive refinement on the MI355X (include/ovr_hip.h: ovr_hip_set_convergence): the estimate changes no
frame, equals the numpy model (ovr_amd.convergence) bit for bit on the renderer's own buffers, the buffers are what they claim (against the CPU oracle, in a child
process on the exact-parity build of the kernels), retired blocks are no longer marched and show A / n_b in both framebuffer sets."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import make_case, oracle_scene, hip_setup, hip_frame
from test_convergence_model import oracle_single_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
CHECK = os.path.join(ROOT, "tests", "convergence_exact_check.py")
PLUGIN = os.path.join(ROOT, "plugin", "libdevice_hip.so")
f32 = np.float32
COUNTERS = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "frame_index", "pipeline", "pool_chunks", "skipped_samples",
            "skipped_shadow_samples", "layout", "stale_tiles", "lds_fallback_taps", "lds_unstaged_rounds", "lds_rounds", "skipping_kernels", "tuning", "replicas_building")


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def new_renderer(ovr, made, group):
    r = ovr.create_renderer("hip", devices=[0, 0]) if group else ovr.create_renderer("hip")
    made.append(r)
    return r


@pytest.fixture
def made():
    rs = []
    yield rs
    for r in rs:
        r.close()


def run_frames(ovr, ren, case, mode, threshold, frames, pipeline, jitter_tile=None, swap=True, layout=0):
    """[(rgba, grad, {counter: value})] of `frames` accumulated frames"""
    if jitter_tile is not None:
        ren.set_noise_tile(jitter_tile)
        ren.set_pixel_jitter(1)
    ren.set_layout_choice(layout)   # (a forced layout and a forced pipeline: nothing is chosen by measured times, the counters are a function of the frame)
    hip_setup(ovr, ren, case, accumulate=True, pipeline=pipeline)
    ren.set_convergence(mode, threshold)
    ren.commit()
    out = []
    for _ in range(frames):
        ren.render()
        rgba, grad = hip_frame(ovr, ren)
        st = ren.stats()
        out.append((rgba, grad, {k: int(getattr(st, k)) for k in COUNTERS}))
        if swap:
            ren.swap()
    return out


# ---- 4. the estimate changes no frame ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", [False, True], ids=["one_renderer", "devices_0_0"])
@pytest.mark.parametrize("pipeline", [1, 2], ids=["in_place", "pooled"])
@pytest.mark.parametrize("sampling", ["spp2_tea", "spp1_blue_noise"])
def test_estimate_mode_changes_no_frame(ovr, oracle, made, sampling, pipeline, group):
    spp = 2 if sampling == "spp2_tea" else 1
    tile = None if sampling == "spp2_tea" else np.random.default_rng(11).random((16, 16, 64), dtype=f32)
    case = make_case(ovr, oracle, n=32, tf="sparse", cam="oblique", size=(100, 76), shading=2, spp=spp)
    runs = [run_frames(ovr, new_renderer(ovr, made, group), case, mode, 0.0, 8, pipeline, tile) for mode in (0, 1)]
    assert runs[0][-1][0].max() > 0
    for n, (a, b) in enumerate(zip(*runs), 1):
        assert same_bits(a[0], b[0]), f"frame {n}: RGBA differs"
        assert same_bits(a[1], b[1]), f"frame {n}: gradient layer differs"
        assert a[2] == b[2], f"frame {n}: counters differ"
    assert runs[0][-1][2]["frame_index"] == 8 and runs[0][-1][2]["samples"] > 0


# ---- 5. the estimate is the model ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["ragged_100x76", "shard_1_3_16", "shard_1_3_12_cuts_blocks", "devices_0_0"])
def test_estimate_equals_the_model(ovr, oracle, made, layout):
    M = ovr.convergence
    W, H = 100, 76
    case = make_case(ovr, oracle, n=32, tf="dense", cam="oblique", size=(W, H), shading=2, spp=2)
    group = layout == "devices_0_0"
    ren = new_renderer(ovr, made, group)
    hip_setup(ovr, ren, case, accumulate=True)
    shards = [(0, 1, 64, 64)]
    if layout.startswith("shard"):
        shards = [(1, 3, 16, 16)] if layout == "shard_1_3_16" else [(1, 3, 12, 12)]
        ren.set_image_shard(*shards[0])
    if group:
        ren.set_image_shard(0, 1, 16, 16)
        shards = [(0, 2, 16, 16), (1, 2, 16, 16)]
    ren.set_convergence(1)
    ren.commit()
    assert ren.convergence().valid == 0 and math.isinf(ren.convergence().error)
    last = None
    for n in range(1, 7):
        ren.render()
        c = ren.convergence()
        if n == 1:
            assert c.valid == 0 and math.isinf(c.error) and ren.variance == float("inf")
            continue
        per_member = []
        for m, shard in enumerate(shards):
            err, frames = ren.convergence_blocks(m)
            per_member.append((err, frames))
            if n % 2:
                continue
            owned = M.owned_mask(W, H, *shard)
            want = M.block_errors(ren.accumulation(0, m), ren.accumulation(1, m), n, owned)
            assert err.shape == want.shape == ((H + 7) // 8, (W + 7) // 8)
            assert same_bits(err, want), f"frame {n}, member {m}: {int((err != want).sum())} block errors differ from the model"
            assert set(np.unique(frames)) <= {0, n} and np.all(frames[want > 0] == n)
            assert (want > 0).sum() >= 4
        if n % 2 == 0:
            assert c.valid == 1 and c.frames == n and c.mode == 1
            assert f32(c.error) == max(e.max() for e, _ in per_member) > 0
            assert ren.variance == float(c.error)
            assert c.blocks == c.active_blocks and c.retired_blocks == 0 and c.blocks >= sum(int((f != 0).sum()) for _, f in per_member) > 0
        else:   # an odd frame: the estimate of the even frame before it stands
            assert c.valid == 1 and c.frames == n - 1
            for (e0, f0), (e1, f1) in zip(last, per_member):
                assert same_bits(e0, e1) and np.array_equal(f0, f1)
        last = per_member


# ---- 6. - 8. against the oracle ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("part", ["buffers", "adaptive", "static"])
def test_exact_against_the_oracle_on_the_parity_instrument(part):
    """tests/convergence_exact_check.py on libovr_hip_parity.so: A and H are the running sums of the oracle's frames; retirement frames are the model's; retired
    blocks show the oracle's A_{n_b} / n_b in both framebuffer sets; a static scene is the oracle's single frame from frame 3 on and marches nothing - bit for bit"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_ORACLE_POWF="det")
    out = subprocess.run([sys.executable, CHECK, part], env=env, capture_output=True, text=True, timeout=900)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "all exact" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_accumulated_frame_with_the_estimate_stays_within_the_parity_bar(ovr, oracle, made):
    """product library: the mapped frame of an accumulation that keeps H is the oracle's accumulated frame to <= 1 on every 8-bit channel"""
    case = make_case(ovr, oracle, n=32, tf="sparse", cam="oblique", size=(100, 76), shading=2, spp=2)
    ren = new_renderer(ovr, made, False)
    hip_setup(ovr, ren, case, accumulate=True)
    ren.set_convergence(1)
    ren.commit()
    for _ in range(4):
        ren.render()
    ref = oracle_scene(oracle, case).render(frames=4, accumulate=True)[0]
    d8 = np.abs(oracle.rgba8(hip_frame(ovr, ren)[0]).astype(int) - oracle.rgba8(ref).astype(int)).max()
    assert d8 <= 1, d8
    A, Hh = ren.accumulation(0), ren.accumulation(1)
    assert np.abs(A / f32(4) - ref).max() <= 2e-4 and Hh.max() > 0 and np.all(Hh <= A + 1e-6)   # (non-negative frames: the half never exceeds the whole)


def test_adaptive_mixed_case_on_the_product(ovr, oracle, made):
    """some blocks retire at once, some later, some never: every retired block has E_b <= t, every active one > t, the mapped pixels are A / n_b of the downloaded
    buffer, the rays counted are those of the blocks that were marched"""
    M = ovr.convergence
    N, W, H = 16, 192, 128
    case = make_case(ovr, oracle, n=32, tf="dense", cam="oblique", size=(W, H), shading=2, spp=2)
    fr = [f[0] for f in oracle_single_frames(oracle, oracle_scene(oracle, case), 4)]
    s = M.accumulate(fr)
    E4 = M.block_errors(s[3][1], s[3][2], 4)
    t = f32(np.median(E4[E4 > 0]))
    ren = new_renderer(ovr, made, False)
    hip_setup(ovr, ren, case, accumulate=True)
    ren.set_convergence(2, float(t))
    ren.commit()
    marched_before = None
    for n in range(1, N + 1):
        ren.render()
        ren.swap()
        st = ren.stats()
        if n % 2 == 0:
            err, frames = ren.convergence_blocks()
            marched = (frames == 0) | (np.abs(frames) == n)    # never estimated (no ray meets them: they keep counting), or marched by this frame
            assert st.rays == 2 * 64 * int(marched.sum()), n
            marched_before = (frames == 0) | (frames == n)
        elif n == 1:
            assert st.rays == 2 * W * H
        else:
            assert st.rays == 2 * 64 * int(marched_before.sum()), n
    ren.swap()   # back to the set of frame N
    rgba = hip_frame(ovr, ren)[0]
    err, frames = ren.convergence_blocks()
    c = ren.convergence()
    retired, active = frames < 0, frames == N
    assert np.all(err[retired] <= t) and np.all(err[active] > t)
    assert set(np.unique(frames[~retired])) <= {0, N}
    assert c.retired_blocks == int(retired.sum()) and c.active_blocks == int(active.sum()) and c.blocks == c.retired_blocks + c.active_blocks
    assert c.error == err.max() > t
    nblk = frames.size
    assert int((retired & (frames < -2)).sum()) >= 0.05 * nblk, "too few blocks retire later than frame 2"
    assert int(active.sum()) >= 0.05 * nblk, "too few blocks are still active"
    A = ren.accumulation(0)
    n_px = np.repeat(np.repeat(np.where(retired, -frames, N), 8, axis=0), 8, axis=1)[:H, :W].astype(f32)
    assert same_bits(rgba, A / n_px[..., None])


@pytest.mark.parametrize("group", [False, True], ids=["one_renderer", "devices_0_0"])
def test_static_scene_on_the_product(ovr, oracle, made, group):
    """one sample per pixel, TEA: every frame is the same frame; threshold 0 retires every block after frame 2, later frames march nothing (a device group: every
    member retires its own tiles' blocks, the leader sums the counts; the retired tiles still travel in the gather)"""
    case = make_case(ovr, oracle, n=32, tf="sparse", cam="oblique", size=(100, 76), shading=2, spp=1)
    S = oracle_scene(oracle, case).render()[0]
    frames = run_frames(ovr, new_renderer(ovr, made, group), case, 2, 0.0, 10, 0, layout=-1)
    ren = made[-1]
    c = ren.convergence()
    assert c.valid == 1 and c.error == 0.0 and c.frames == 2 and c.active_blocks == 0 and c.retired_blocks == c.blocks > 0
    assert ren.variance == 0.0
    for n, (rgba, grad, st) in enumerate(frames, 1):
        assert np.abs(oracle.rgba8(rgba).astype(int) - oracle.rgba8(S).astype(int)).max() <= 1, n
        assert same_bits(rgba, frames[0][0]) and same_bits(grad, frames[0][1]), n     # (S + S) / 2 == S: the retired pixels are frame 1's
        assert (st["samples"] == 0) == (n >= 3), (n, st)
        assert st["frame_index"] == n
    empty_rays = frames[-1][2]["rays"]
    assert frames[0][2]["rays"] == 100 * 76 and 0 <= empty_rays < 100 * 76 and frames[-1][2]["active_pixels"] == empty_rays


def test_adaptive_frames_do_not_depend_on_how_they_are_launched(ovr, oracle, made):
    """ovr_hip_render_async + ovr_hip_sync (the active count of frame n reaches the host when frame n is resolved, before frame n + 1 is launched) and a device
    group give the frames, errors and retirement frames of blocking renders on one renderer"""
    M = ovr.convergence
    case = make_case(ovr, oracle, n=32, tf="dense", cam="oblique", size=(100, 76), shading=2, spp=2)
    fr = [f[0] for f in oracle_single_frames(oracle, oracle_scene(oracle, case), 4)]
    s = M.accumulate(fr)
    E4 = M.block_errors(s[3][1], s[3][2], 4)
    t = float(np.median(E4[E4 > 0]))
    results = []
    for how in ("blocking", "async", "group"):
        ren = new_renderer(ovr, made, how == "group")
        hip_setup(ovr, ren, case, accumulate=True)
        if how == "group":
            ren.set_image_shard(0, 1, 8, 8)   # tiles of whole blocks: a block belongs to one member, so the members' blocks are the single renderer's
        ren.set_convergence(2, t)
        ren.commit()
        for _ in range(8):
            if how == "async":
                ren.render_async()
                ren.sync()
            else:
                ren.render()
            ren.swap()
        ren.swap()
        rgba, grad = hip_frame(ovr, ren)
        members = [ren.convergence_blocks(m) for m in range(2 if how == "group" else 1)]
        err = np.maximum.reduce([e for e, _ in members])
        frames = np.where(members[0][1] != 0, members[0][1], members[-1][1])
        c = ren.convergence()
        results.append((rgba, grad, err, frames, (c.valid, c.frames, c.retired_blocks, c.active_blocks), c.error))
    a = results[0]
    assert (a[3] < 0).sum() > 0 and (a[3] == 8).sum() > 0
    for b in results[1:]:
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4] and a[5] == b[5]


# ---- 9. state ---------------------------------------------------------------------------------------------------------------------------------------------

def test_resets_and_modes(ovr, oracle, made):
    lib = ovr._lib.load()
    case = make_case(ovr, oracle, n=32, tf="sparse", cam="oblique", size=(96, 64), shading=2, spp=1)
    ren = new_renderer(ovr, made, False)
    hip_setup(ovr, ren, case, accumulate=True)
    ren.set_convergence(2, 0.0)
    ren.commit()

    def retire_all():
        ren.render()
        c = ren.convergence()
        assert c.valid == 0 and math.isinf(c.error) and c.retired_blocks == 0 and c.active_blocks == c.blocks > 0 and ren.stats().samples > 0
        ren.render()
        c = ren.convergence()
        assert c.valid == 1 and c.retired_blocks == c.blocks > 0 and c.active_blocks == 0
        ren.render()
        assert ren.stats().samples == 0

    retire_all()
    eye, at, up = case["cam"]
    changes = [
        lambda: ren.set_camera(tuple(1.1 * np.array(eye)), at, up),
        lambda: ren.set_transfer_function(case["colors"], case["alphas"] * np.float32(0.5), case["vr"]),
        lambda: ren.set_fbsize((104, 72)),
        lambda: ren.set_convergence(2, 0.0),
        lambda: ren.set_convergence(2, 0.5),
        lambda: ren.set_convergence(1, 0.0),
        lambda: ren.set_convergence(2, 0.0),
    ]
    for k, change in enumerate(changes):
        change()
        ren.commit()
        c = ren.convergence()
        assert c.valid == 0 and math.isinf(c.error) and c.retired_blocks == 0, k
        if k == 5:   # estimate only: nothing retires
            ren.render(); ren.render(); ren.render()
            c = ren.convergence()
            assert c.valid == 1 and c.retired_blocks == 0 and ren.stats().samples > 0
        else:
            retire_all()
    # bad arguments: EINVAL, nothing changes
    before = ren.convergence()
    for mode, thr in ((3, 0.0), (-1, 0.0), (2, -0.5), (1, float("nan")), (2, float("inf"))):
        assert lib.ovr_hip_set_convergence(ren._h, mode, C.c_float(thr)) == -1
    ren.commit()
    after = ren.convergence()
    assert (after.valid, after.mode, after.threshold, after.retired_blocks, after.frames) == (before.valid, before.mode, before.threshold, before.retired_blocks, before.frames) and after.valid == 1
    with pytest.raises(RuntimeError, match="unknown mode"):
        ren.set_convergence(7)


@pytest.mark.parametrize("what", ["sparse_sampling", "no_accumulation"])
def test_undefined_without_accumulation_or_with_sparse_sampling(ovr, oracle, made, what):
    case = make_case(ovr, oracle, n=32, tf="sparse", cam="oblique", size=(96, 64), shading=2, spp=1)
    tile = np.random.default_rng(3).random((16, 16, 64), dtype=f32)
    got = []
    for mode in (0, 2):
        ren = new_renderer(ovr, made, False)
        ren.set_noise_tile(tile)
        hip_setup(ovr, ren, case, accumulate=what == "sparse_sampling")
        if what == "sparse_sampling":
            ren.set_focus((0.5, 0.5), 0.4, 0.2)
            ren.set_sparse_sampling(True)
        ren.set_convergence(mode, 0.0)
        ren.commit()
        frames = []
        for _ in range(4):
            ren.render()
            frames.append(hip_frame(ovr, ren) + (ren.stats().samples,))
            c = ren.convergence()
            assert c.valid == 0 and math.isinf(c.error) and c.retired_blocks == 0
            assert ren.variance == (float("inf") if mode else 0.0)
        got.append(frames)
    for a, b in zip(*got):
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2] == b[2] > 0


def test_pool_overflow_changes_nothing(tmp_path):
    """OVR_HIP_POOL_CHUNKS=8 (the existing diagnostic) makes the first pooled frame overflow the request pool - in the child that is frame 2, the first one with an
    estimate behind it (frame 1 is shaded in place): it is rendered again, and the frames, the block errors and the retirement frames of the adaptive run are those
    of a run without the overflow (the overflowing attempt wrote no pixel, estimated nothing and retired nothing)"""
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
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 8 * 6
    for k in a.files:
        assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == f32 else a[k], b[k].view(np.uint32) if b[k].dtype == f32 else b[k]), k
    assert (a["frames8"] < 0).sum() > 0 and (a["frames8"] == 8).sum() > 0 and len(set(np.unique(a["frames8"]))) >= 4


# ---- 10. the plugin ---------------------------------------------------------------------------------------------------------------------------------------

def _probe_env(tmp_path, **extra):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.dirname(PLUGIN), os.path.join(ROOT, "open-volume-renderer_amd"), env.get("LD_LIBRARY_PATH", "")])
    for k in ("OVR_HIP_CONVERGENCE", "OVR_HIP_CONVERGENCE_THRESHOLD", "OVR_HIP_QUIET"):
        env.pop(k, None)
    env.update(extra)
    return env


def test_plugin_variables(tmp_path, ovr):
    probe = os.path.join(ROOT, "oracle", "_ref", "plugin_probe")
    if not (os.path.exists(probe) and os.path.exists(PLUGIN)):
        pytest.skip("oracle/_ref/plugin_probe or plugin/libdevice_hip.so missing (built by __graft_entry__.build() where the reference tree is present)")
    n, W, H = 40, 112, 72
    vol = ovr.synth.make_volume(n, np.float32)
    colors, alphas, vr = ovr.synth.make_tfn("bumps", 256)
    cam = ovr.synth.make_camera("oblique", n)
    scene_path = ovr.vidi3d.write_scene(str(tmp_path), "synthetic", vol, ovr.synth._RAINBOW, alphas[1::2].copy(), (0.0, 1.0), cam, fovy=45.0, sample_distance=0.5)
    np.random.default_rng(7).random((32, 32, 64), dtype=np.float32).tofile(str(tmp_path / "noise.bin"))
    dumps = []
    for k, extra in enumerate(({}, {"OVR_HIP_CONVERGENCE": "1"})):
        env = _probe_env(tmp_path, OVR_HIP_NOISE_TILE=str(tmp_path / "noise.bin"), **extra)
        out = subprocess.run([probe, scene_path, str(W), str(H), str(tmp_path / f"frames{k}.f32")], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert ("[hip] convergence:" in out.stderr) == bool(extra)
        dumps.append(open(tmp_path / f"frames{k}.f32", "rb").read())
    assert dumps[0] == dumps[1] and len(dumps[0]) == 2 * W * H * 16
    env = _probe_env(tmp_path, OVR_HIP_CONVERGENCE="2")
    out = subprocess.run([probe, "--loop", "40", scene_path, str(W), str(H)], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "loop fps" in out.stdout, out.stdout + out.stderr
    m = re.search(r"\[hip\] convergence: error (\S+) after (\d+) frames, (\d+) of (\d+) blocks retired", out.stderr)
    assert m, out.stderr
    assert float(m.group(1)) == 0.0 and int(m.group(2)) == 2 and int(m.group(3)) == int(m.group(4)) > 0
