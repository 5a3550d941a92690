"""The host-upload path at a size where it takes more than one slab, with a seam that cuts a brick layer.

ovr_hip_set_volume stages a HOST array through a device buffer of at most 1 GiB, slab by slab, and the relayout kernels take (z0, nz_chunk) so that a brick layer
cut by a slab boundary is written half by each launch and padding rows exactly once.  Every volume the reference's renderbatch loads takes this path, yet every
other test either uploads from device memory or fits one slab, and the full-size volumes' slabs (256 / 128 slices) are brick-aligned.  Here all dimensions are odd
and the slab - 2^30 / (nx * ny * sizeof(voxel)) slices - is a multiple of neither the brick's z extent nor a 32-slice macro block."""
import numpy as np
import pytest

from helpers import compare, hip_frame, hip_setup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype,dims,slab", [("float32", (800, 600, 700), 559), ("uint16", (901, 700, 1000), 851), ("uint8", (1100, 999, 1100), 977)])
def test_host_upload_in_ragged_slabs(ovr, oracle, hip_renderer_factory, monkeypatch, dtype, dims, slab):
    import torch
    monkeypatch.setenv("OVR_HIP_POISON_ALLOC", "1")   # a fresh layout starts as 0xff bytes: an element no launch wrote shows as NaN / the type's extreme
    nx, ny, nz = dims
    npdt = np.dtype(dtype)
    assert slab == (1 << 30) // (nx * ny * npdt.itemsize) and slab < nz and slab % 2 == 1 and slab % 32 != 0
    if dtype == "uint16" and not hasattr(torch, "uint16"):
        pytest.skip("no torch.uint16")
    full = ovr.synth.make_volume_torch(max(dims), "cuda:0", dtype)
    vol_d = full[:nz, :ny, :nx].contiguous()
    del full
    torch.cuda.empty_cache()
    vol_h = (vol_d.view(torch.int16).cpu().numpy().view(np.uint16) if dtype == "uint16" else vol_d.cpu().numpy())
    assert vol_h.shape == (nz, ny, nx) and vol_h.dtype == npdt and 1.2e9 < vol_h.nbytes < 1.45e9

    colors, alphas, vr = ovr.synth.make_tfn("sparse", 256, npdt)
    up = (0.0, 1.0, 0.0)
    # looks along the seam: the eye beside the box at the height of the slab boundary, the rays fan out around the plane z = slab
    seam = ((-0.35 * nx, 0.5 * ny, slab + 0.5), (0.5 * nx, 0.5 * ny, float(slab)), up)
    centre, d = np.array([0.5 * nx, 0.5 * ny, 0.5 * nz]), np.array([-0.82, 0.41, 0.40])
    overview = (tuple(centre + 1.9 * max(dims) * d / np.linalg.norm(d)), tuple(centre), up)   # the whole box, obliquely
    base = dict(colors=colors, alphas=alphas, vr=vr, shading=2, rate=1.0, spp=1, convention=0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), fovy=60.0)

    rens = {}
    for where, vol in (("device", vol_d), ("host", vol_h)):
        ren = hip_renderer_factory()
        ren.set_volume_layouts(2)   # every layout resident when the upload returns
        hip_setup(ovr, ren, dict(base, vol=vol, cam=seam, size=(64, 48)))
        rens[where] = ren
    info = {k: r.volume_info() for k, r in rens.items()}
    assert (info["host"].data_lower, info["host"].data_upper) == (info["device"].data_lower, info["device"].data_upper)
    assert tuple(info["host"].dims) == dims
    mm_d, mj_d = rens["device"].macrocells()
    mm_h, mj_h = rens["host"].macrocells()
    assert np.array_equal(mm_h, mm_d) and np.array_equal(mj_h, mj_d), "macrocell grids differ between the host and the device upload"

    seam_frame = None
    for cam, size in ((seam, (64, 48)), (overview, (128, 96))):
        for choice in (0, 1, 2, 3):
            got = {}
            for where, ren in rens.items():
                ren.set_fbsize(size)
                ren.set_camera(ovr.Camera(*cam, 60.0))
                ren.set_layout_choice(choice)
                ren.commit()
                ren.render()
                got[where] = hip_frame(ovr, ren)
            tag = f"{dtype} {dims} layout {choice} {'seam' if cam is seam else 'overview'}"
            assert np.isfinite(got["host"][0]).all() and np.isfinite(got["host"][1]).all(), tag
            assert np.array_equal(got["host"][0].view(np.uint32), got["device"][0].view(np.uint32)), f"{tag}: rgba differs between the host and the device upload"
            assert np.array_equal(got["host"][1].view(np.uint32), got["device"][1].view(np.uint32)), f"{tag}: grad differs between the host and the device upload"
            assert (got["host"][0][..., 3] > 0).mean() > 0.01, tag   # (a sanity check on the camera only: the table hides all but the field's two blobs)
            if cam is seam and choice == 0:
                seam_frame = got["host"][0]
    for r in rens.values():
        r.close()
    del vol_d
    torch.cuda.empty_cache()

    # the oracle on the seam frame (zero-opacity samples unshaded: bit-identical frames, oracle.py)
    sc = oracle.OracleScene(vol_h, colors, alphas, vr, seam, 64, 48, fovy=60.0, shading=oracle.SHADE_FULL, skip_zero_opacity=True)
    ref, _, cnt = sc.render()
    assert cnt.shaded_samples > 1000
    compare(oracle, seam_frame, ref, name=f"{dtype} {dims} seam frame vs oracle")
