"""Inputs shared by tests/test_frame_machinery_model.py (no GPU) and tests/test_frame_machinery_gpu.py: the table of the eight newer frame kinds and the inputs of
the host machinery they are taken through (the sparse sample list, pull-push filling, image shards, accumulation, ESTIMATE, ADAPTIVE, ovr_hip_update_volume).
Nothing here loads the HIP library: a row's `start` calls the setters of the renderer it is handed, its `model` and `check` are the feature test's own `_model`
and `_check_frame`, imported - the bars stay where those files put them - and its case is the feature's committed one where the list below does not say otherwise.

THE KINDS.  Every volume is projection_cases' float32 `smooth` one, 40 x 33 x 18:
  1 slices          test_slices_gpu's case (its `sparse` table, the oblique camera, rate 1) under SETS["orthogonal"]: three planes
  2 slab            the same case under the 9-voxel MAXIMUM slab of test_range_skipping_is_invisible, empty-space skipping committed: the walk kernel's skipping twin
  3 context         slice_context_cases' SLICES (a plane and a 3-voxel MAXIMUM slab) behind a FRONT context of scale 1 at its rate 0.5, under the AXIS camera and
                    preintegration_cases' `dense` table over the smooth volume's range.  (The committed case - the `random` volume from the oblique camera - leaves
                    2 of its blocks active after 8 ADAPTIVE frames, the condition asks for 3; from the axis camera the model leaves 11, and none of its 487 met rays
                    is borderline.)
  4 preintegrated   preintegration_cases' committed case (the `ones` table, the axis camera, rate 1)
  5 gradient        gradient_opacity_cases' committed case, shading GRADIENT
  6 limited         max_depth_cases' committed case, shading GRADIENT, plane_image of the frame's size
  7 depth           depth_output_cases' committed case, tau 0.5, shading NONE, no depth image
  8 depth-limited   the same, shading GRADIENT, with plane_image: the `limited` path
A model frame is (rgba, layer, counters) for every kind (the pre-integrated model has no layer: its layer is zero, as _check_frame asserts of the device's).

THE UPDATE.  The box (BOX_LOWER, BOX_SHAPE) lies at the centre of the smooth volume's blob and covers about 40 pixels of the 40 x 28 frame; the test asks that more
than UPDATE_PIXELS of them change.  Under the `ones` table every ray is opaque long before it reaches the box - the models of the volume and of the patched volume
are equal bit for bit, and an update that did nothing would pass -, and the three orthogonal planes pass beside it.  A row's `update` is therefore the row the
update test runs: kinds 4 ... 8 under preintegration_cases' `dense` table (alpha 0.9 i / 15: the rays reach the box, 42 pixels change in every model), kind 1 as
slice_context_cases' plane through the centre under the axis camera (36 pixels); kinds 2 and 3 as they are (32 and 33 pixels).
tests/test_frame_machinery_model.py asserts these counts' bar on the models."""
import numpy as np

import depth_output_cases as DC
import max_depth_cases as MC
import preintegration_cases as QC
import projection_cases as PC
import slice_context_cases as CC
import test_depth_output_gpu as TD
import test_gradient_opacity_gpu as TG
import test_max_depth_gpu as TM
import test_preintegration_gpu as TQ
import test_slice_context_gpu as TX
import test_slices_gpu as TS

F = np.float32
SMALL = PC.SIZE            # 40 x 28, ragged 8 x 8 blocks: sparse sampling, ESTIMATE, the update
LARGE = (56, 40)           # 7 x 5 whole blocks; under 16 x 8 tiles it splits three ways: shards, ADAPTIVE
TILE = (16, 8)
WORLD = 3
FOCUS = ((0.5, 0.5), 0.3, 0.2)
SPARSE_FRAMES = 4
ESTIMATE_FRAMES = 6
ADAPTIVE_FRAMES = 8
THRESHOLD_FRAME = 4        # the ADAPTIVE threshold: the median of the positive block errors of the MODEL's frames 1 ... 4
RETIRED_MIN, LATE_MIN, ACTIVE_MIN = 3, 1, 3      # of the 35 blocks after frame 8: retired, retired later than frame 2, still active
BOX_LOWER = (14, 12, 8)    # (x, y, z); the box is 11 x 9 x 6 voxels: unaligned, across brick and macrocell borders (test_projection_gpu's)
BOX_SHAPE = (6, 9, 11)     # (nz, ny, nx)
UPDATE_PIXELS = 30         # the patched frame differs from the frame before in more pixels than this
LIT_PIXELS = 100
SLAB = [(TS.CENTRE, (0.1, 0.2, 1.0), 9.0, TS.MAXIMUM)]
_memo = {}


def noise_tile():
    if "noise" not in _memo:
        _memo["noise"] = np.random.default_rng(77).random((16, 16, 64)).astype(F)
        _memo["noise"].setflags(write=False)
    return _memo["noise"]


def indicator(oracle, frame_index, size):
    """the ORACLE's sample list of a frame as an (H, W) 0 / 1 plane (test_reconstruction_gpu.indicator under this file's tile and focus)"""
    key = ("list", frame_index, size)
    if key not in _memo:
        w, h = size
        xy = oracle.sparse_mask(frame_index, w, h, FOCUS[0], FOCUS[1], FOCUS[2], noise_tile()).reshape(-1, 2)
        m = np.zeros((h, w), F)
        m[xy[:, 1], xy[:, 0]] = 1
        assert int(m.sum()) == len(xy)      # the list holds a pixel at most once
        m.setflags(write=False)
        _memo[key] = m
    return _memo[key]


def patch_volume(vol, value):
    """(patch, patched volume): the box of BOX_SHAPE at BOX_LOWER set to `value`"""
    patch = np.full(BOX_SHAPE, value, vol.dtype)
    patched = vol.copy()
    x, y, z = BOX_LOWER
    patched[z:z + BOX_SHAPE[0], y:y + BOX_SHAPE[1], x:x + BOX_SHAPE[2]] = patch
    return patch, patched


class ModelRenderer:
    """what a feature test's `_model` asks of its renderer, without one: the camera basis of the case (camera.basis, which tests/test_camera_model.py holds to
    the device's) and no node table (preintegration.frame then builds the model's own, which tests/test_preintegration_host.py holds to the library's)"""

    class _Camera:
        pass

    def __init__(self, ovr, case):
        c = self._Camera()
        c.pos, c.dir, c.hor, c.ver = ovr.camera.basis(*case["cam"], *case["size"], fovy=case["fovy"])
        self._camera = c

    def get_camera(self):
        return self._camera

    def preintegration_tables(self):
        return None


class Kind:
    """a row of the table.  case(ovr, size, vol): the helpers.hip_setup case (vol: another volume than the kind's own); start(ren, size): the kind's own setters
    and the commit, after hip_setup; model(ovr, ren, case, **kw): (rgba, layer, counters) - ren: the renderer or a ModelRenderer; check(ovr, oracle, ren, case,
    got, want, tag): the feature's _check_frame; update: the row the update test runs (see THE UPDATE above), by default the row itself"""
    name = None
    layer = "gradient"      # what the frame's layer holds: "gradient", "slice" (v, t, k), "depth" (d, S, reached), "zero"
    skipping = False
    plane = False           # a committed depth image: plane_image of the frame's size
    patch = 0.97            # the value of the update's box: above every voxel of the `smooth` volume

    def __init__(self, update=None, **over):
        self.over = over
        self.key = (self.name, repr(sorted(over.items())), repr(getattr(self, "slices", None)))
        self.update = self if update is None else type(self)(**update)

    def volume(self):
        return PC.volume("smooth", np.float32)

    def case(self, ovr, size, vol=None):
        return self._case(ovr, self.volume() if vol is None else vol, size=size, **self.over)

    def depth(self, size):
        return MC.plane_image(size) if self.plane else None

    def begin(self, ovr, ren, case, accumulate=False, jitter=False, noise=False):
        """hip_setup under a forced layout (nothing is chosen by measured times: the counters are a function of the frame), then the kind"""
        from helpers import hip_setup
        ren.set_layout_choice(0)
        if noise or jitter:
            ren.set_noise_tile(noise_tile())
        if jitter:
            ren.set_pixel_jitter(1)
        hip_setup(ovr, ren, case, accumulate=accumulate)
        self.start(ren, case["size"])
        return ren


class Slices(Kind):
    name, layer = "slices", "slice"
    slices = TS.SETS["orthogonal"]

    def __init__(self, update=None, slices=None, **over):
        if slices is not None:
            self.slices = slices
        Kind.__init__(self, update, **over)

    def _case(self, ovr, vol, **kw):
        return TS._case(ovr, vol, **kw)

    def start(self, ren, size):
        ren.set_slices(self.slices)
        ren.set_empty_space_skipping(self.skipping)
        ren.commit()

    def model(self, ovr, ren, case, **kw):
        return TS._model(ovr, ren, case, self.slices, skipping=self.skipping, **kw)

    def check(self, ovr, oracle, ren, case, got, want, tag):
        TS._check_frame(case, got, want, tag, skipping=self.skipping)


class Slab(Slices):
    name, slices, skipping = "slab", SLAB, True


class Context(Kind):
    name, layer, skipping = "context", "slice", True

    def _case(self, ovr, vol, **kw):
        case = TX._case(ovr, vol, **kw)
        colors, alphas, vr = QC.transfer_function(ovr, "dense", vol.dtype, "smooth")      # (slice_context_cases' `dense` table spans its `random` volume's range)
        case.update(colors=colors, alphas=alphas, vr=vr)
        return case

    def start(self, ren, size):
        ren.set_slices(CC.SLICES)
        ren.set_slice_context(TX.FRONT, 1.0)
        ren.set_empty_space_skipping(True)      # committed, and ignored: the context fetches every sample
        ren.commit()

    def model(self, ovr, ren, case, **kw):
        return TX._model(ovr, ren, case, CC.SLICES, **kw)

    def check(self, ovr, oracle, ren, case, got, want, tag):
        TX._check_frame(ovr, oracle, case, got, want, tag)


class Preintegrated(Kind):
    name, layer = "preintegrated", "zero"

    def _case(self, ovr, vol, **kw):
        return TQ._case(ovr, vol, **kw)

    def start(self, ren, size):
        ren.set_preintegration(TQ.SEGMENTS)
        ren.commit()

    def model(self, ovr, ren, case, **kw):
        rgba, cnt = TQ._model(ovr, ren, case, **kw)
        return rgba, np.zeros(rgba.shape[:2] + (3,), F), cnt

    def check(self, ovr, oracle, ren, case, got, want, tag):
        TQ._check_frame(ovr, oracle, case, got, (want[0], want[2]), tag)


class Gradient(Kind):
    name = "gradient"

    def _case(self, ovr, vol, **kw):
        return TG._case(ovr, vol, shading=1, **kw)

    def start(self, ren, size):
        TG._lit(ren)
        ren.set_gradient_opacity(TG.RAMP, *TG.GC.RAMP_CASE)
        ren.commit()

    def model(self, ovr, ren, case, **kw):
        return TG._model(ovr, ren, case, **kw)

    def check(self, ovr, oracle, ren, case, got, want, tag):
        TG._check_frame(oracle, got, want, tag)


class Limited(Kind):
    name, plane = "limited", True

    def _case(self, ovr, vol, **kw):
        return TM._case(ovr, vol, shading=1, **kw)

    def start(self, ren, size):
        TM._lit(ren)
        ren.set_max_depth(self.depth(size))      # the image of the whole frame, whatever part of it the renderer draws
        ren.commit()

    def model(self, ovr, ren, case, **kw):
        return TM._model(ovr, ren, case, self.depth(case["size"]), **kw)

    def check(self, ovr, oracle, ren, case, got, want, tag):
        TM._check_frame(oracle, got, want, tag)


class Depth(Kind):
    name, layer, shading, tau = "depth", "depth", 0, 0.5

    def _case(self, ovr, vol, **kw):
        return TD._case(ovr, vol, shading=self.shading, **kw)

    def start(self, ren, size):
        TD._lit(ren)
        ren.set_max_depth(self.depth(size))
        ren.set_depth_output(self.tau)
        ren.commit()

    def model(self, ovr, ren, case, **kw):
        return TD._model(ovr, ren, case, self.tau, self.depth(case["size"]), **kw)

    def check(self, ovr, oracle, ren, case, got, want, tag):
        TD._check_frame(oracle, got, want, tag, TD._t1max(ren))


class DepthLimited(Depth):
    name, shading, plane = "depth-limited", 1, True


DENSE = dict(tf="dense")
KINDS = (Slices(update=dict(cam="axis", slices=[CC.SLICES[0]])), Slab(), Context(cam="axis"), Preintegrated(update=DENSE), Gradient(update=DENSE), Limited(update=DENSE), Depth(update=DENSE),
         DepthLimited(update=DENSE))
IDS = [k.name for k in KINDS]


def model_frame(ovr, kind, size, frame_index=None, vol=None, ren=None):
    """the kind's model frame (rgba, layer, counters), memoized: frame_index None is the dense frame of the pixel centres, k >= 1 the frame of one sample per
    pixel under the blue-noise jitter; vol: the patched volume of the update test (keyed "patched").  ren: a renderer whose camera and node table the feature's
    _model reads; without one a ModelRenderer stands in"""
    key = ("model", kind.key, size, frame_index, vol is not None, ren is not None)
    if key not in _memo:
        case = kind.case(ovr, size, vol)
        kw = {} if frame_index is None else dict(noise=noise_tile(), frame_index=frame_index)
        _memo[key] = kind.model(ovr, ModelRenderer(ovr, case) if ren is None else ren, case, **kw)
    return _memo[key]


def threshold(ovr, kind, frames):
    """the ADAPTIVE threshold from the first THRESHOLD_FRAME of `frames` (rgba per frame): the median of the positive block errors"""
    M = ovr.convergence
    _, A, H = M.accumulate(frames[:THRESHOLD_FRAME])[-1]
    E = M.block_errors(A, H, THRESHOLD_FRAME)
    return float(np.median(E[E > 0]))


def block_hit(frames):
    """(by, bx) bool: the blocks in which some frame has a non-zero pixel (the others have E_b = 0 whether or not they are marched)"""
    total = np.abs(np.asarray(frames, F)).sum(axis=(0, -1)) != 0
    h, w = total.shape
    return total.reshape(h // 8, 8, w // 8, 8).any(axis=(1, 3))


def adaptive_condition(n_b, hit, last):
    """n_b: the even frame after which a block retired, 0 = still active after frame `last`"""
    retired, late, active = int(((n_b > 0) & hit).sum()), int(((n_b > 2) & hit).sum()), int(((n_b == 0) & hit).sum())
    assert retired >= RETIRED_MIN and late >= LATE_MIN and active >= ACTIVE_MIN, (retired, late, active)
    return retired, late, active
