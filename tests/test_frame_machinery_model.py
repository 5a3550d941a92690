"""The conditions tests/test_frame_machinery_gpu.py rests on, shown on the references alone (no GPU): the oracle's sample lists leave both listed pixels and
holes, every kind's model frame is lit, the depth kinds' layers hold reached and unreached pixels, the update's box changes the model frame, and under the
threshold the ADAPTIVE test derives from the model's frames 1 ... 4 the model's own frames 1 ... 8 retire some blocks at frame 2, some later and leave some
active - so that none of the equalities over there holds between empty frames, or between frames no block of which ever retired."""
import numpy as np
import pytest

import frame_machinery_cases as FM

f32 = np.float32


def _differing_pixels(a, b):
    bits = lambda x: np.ascontiguousarray(x, f32).view(np.uint32)
    return int(((bits(a[0]) != bits(b[0])).any(-1) | (bits(a[1]) != bits(b[1])).any(-1)).sum())


def test_the_oracles_lists_leave_samples_and_holes(oracle):
    w, h = FM.SMALL
    N = np.zeros((h, w), f32)
    counts = []
    for k in range(1, FM.SPARSE_FRAMES + 1):
        m = FM.indicator(oracle, k, FM.SMALL)
        counts.append(int(m.sum()))
        N += m
    print("listed pixels per frame", counts, "of", w * h)
    assert all(50 <= c <= w * h - 50 for c in counts), counts
    assert len(set(counts)) > 1 or not np.array_equal(FM.indicator(oracle, 1, FM.SMALL), FM.indicator(oracle, 2, FM.SMALL))      # the list depends on the frame
    assert N.max() >= 2 and (N == 0).any()


@pytest.mark.parametrize("kind", FM.KINDS, ids=FM.IDS)
def test_dense_model_frames_are_lit(ovr, kind):
    for row, size in ((kind, FM.SMALL), (kind, FM.LARGE), (kind.update, FM.SMALL)):
        rgba, layer, cnt = FM.model_frame(ovr, row, size)
        assert rgba.shape == size[::-1] + (4,) and layer.shape == size[::-1] + (3,) and not np.isnan(rgba).any()
        lit = int((rgba[..., 3] > 0).sum())
        assert lit > FM.LIT_PIXELS and lit < size[0] * size[1], (row.key, size, lit)      # and a background: the frame is not one value
        if row.layer == "zero":
            assert not layer.any()
        else:
            assert layer.any(), (row.key, size)
        if row.layer == "depth":      # (d, S, reached): both reached and unreached lit pixels
            reached = layer[..., 2] == 1
            assert reached.sum() > 50 and ((rgba[..., 3] > 0) & ~reached).sum() > 50 and (layer[..., 0][reached] > 0).all() and not layer[..., 0][~reached].any(), (row.key, size)
        if row.layer == "slice":
            assert (layer[..., 2] >= 1).sum() > 50, (row.key, size)
        if row.plane:      # the depth image cuts rays, and leaves others alone
            image = row.depth(size)
            assert np.isfinite(image).sum() > 100 and (~np.isfinite(image)).sum() > 20


@pytest.mark.parametrize("kind", FM.KINDS, ids=FM.IDS)
def test_the_updates_box_changes_the_model_frame(ovr, kind):
    row = kind.update
    vol = row.volume()
    patch, patched = FM.patch_volume(vol, row.patch)
    x, y, z = FM.BOX_LOWER
    around = vol[z - 1:z + FM.BOX_SHAPE[0] + 1, y - 1:y + FM.BOX_SHAPE[1] + 1, x - 1:x + FM.BOX_SHAPE[2] + 1]
    assert float(patch.min()) > float(around.max()) and not np.array_equal(patched, vol)      # brighter than its surroundings
    assert any(a % 8 and (a + n) % 8 and a // 8 != (a + n) // 8 for a, n in zip(FM.BOX_LOWER, FM.BOX_SHAPE[::-1]))      # unaligned, across a brick border
    before, after = FM.model_frame(ovr, row, FM.SMALL), FM.model_frame(ovr, row, FM.SMALL, vol=patched)
    changed = _differing_pixels(before, after)
    print(row.key, "pixels the box changes in the model frame:", changed)
    assert changed > FM.UPDATE_PIXELS, (row.key, changed)


@pytest.mark.parametrize("kind", FM.KINDS, ids=FM.IDS)
def test_adaptive_condition_on_the_models_frames(ovr, kind):
    """the threshold of the GPU test, and under it the model's own eight frames: at least 3 blocks retire, at least 1 of them later than frame 2, at least 3 stay
    active (blocks no ray lights are not counted: their error is 0 whatever happens to them)"""
    M = ovr.convergence
    frames = [FM.model_frame(ovr, kind, FM.LARGE, k)[0] for k in range(1, FM.ADAPTIVE_FRAMES + 1)]
    assert not any(np.array_equal(frames[0], f) for f in frames[1:])      # the jitter moves every frame
    t = FM.threshold(ovr, kind, frames)
    n_b, E_b, image = M.retirement_frames(frames, t)
    hit = FM.block_hit(frames)
    got = FM.adaptive_condition(n_b, hit, FM.ADAPTIVE_FRAMES)
    print(kind.key, "threshold", t, "lit blocks", int(hit.sum()), "of", hit.size, "retired / later than frame 2 / active", got)
    assert t > 0 and n_b.shape == (FM.LARGE[1] // 8, FM.LARGE[0] // 8) == hit.shape and hit.size == 35
