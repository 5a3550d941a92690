"""shared by the tests that read tests/golden/ref_march.npz: the sparse scene's noise tile, a fixture scene through the HIP device"""
import os

import numpy as np

import ref_march_scenes as RS

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ref_march.npz")


def noise_tile_for(scene):
    """a noise tile with which the sparse mask (keep a pixel iff noise < p, p in [0.1, 1]) is exactly the scene's pixel list"""
    xy = 32
    w, h = scene["size"]
    assert w <= xy and h <= xy
    tile = np.ones((xy, xy, 64), np.float32)
    tile[scene["pixels"][:, 1], scene["pixels"][:, 0], :] = 0.0
    return tile


def hip_render(ovr, ren, s, pipeline=0, skip=False):
    """-> rgba, grad of the last frame, primary samples (marched + skipped) and shadow samples (marched + skipped) summed over all frames"""
    sparse = len(s["pixels"]) > 0
    scene = ovr.Scene(volume=s["vol"], grid_origin=tuple(s["origin"]), grid_spacing=tuple(s["spacing"]), transfer_function=None, volume_sampling_rate=s["rate"])
    eye, at, up = (tuple(float(x) for x in v) for v in s["cam"])
    ren.set_fbsize(tuple(s["size"]))
    ren.set_frame_accumulation(bool(s["accumulate"]))
    ren.set_sample_per_pixel(s["spp"])
    ren.set_volume_sampling_rate(s["rate"])
    ren.set_shading(2)
    ren.set_shading_pipeline(pipeline)
    ren.set_grid_convention(0)
    ren.set_transfer_function(s["colors"], s["alphas"], s["vr"])
    if sparse:
        ren.set_noise_tile(noise_tile_for(s))
        ren.set_focus((0.5, 0.5), 0.2, 0.1)
    ren.init(scene, ovr.Camera(eye, at, up, s["fovy"]))
    ren.set_sparse_sampling(sparse)
    ren.set_empty_space_skipping(skip)
    ren.commit()
    primary = shadow = 0
    for _ in range(s["frames"]):
        ren.render()
        st = ren.stats()
        primary += int(st.samples) + int(st.skipped_samples)
        shadow += int(st.shadow_samples) + int(st.skipped_shadow_samples)
    fb = ovr.FrameBufferData()
    ren.mapframe(fb)
    return np.array(fb.rgba.data(), copy=True), np.array(fb.grad.data(), copy=True), primary, shadow
