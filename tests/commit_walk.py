"""The walk of tests/test_commit_effects_gpu.py and tools/commit_states.py: every source of csrc/host/commit_plan.hpp's table applied to one renderer through
the C binding (no wrapper between the caller and the setter: a repeated value reaches the library), with a new value and with the same value again, and
what an application can see of it - ovr_hip_stats.frame_index of the frame after the commit and the shadow cache's build count.

A 24^3 f32 volume, a 96 x 64 frame, accumulation on, full shading, shadow mode CACHED (cell 4).  One step: set the camera to what it is and commit (the
accumulation starts over), render three frames (frame_index 3), apply the step, commit, render one frame.  The step's literals: `index` - 1 where the
accumulation starts over, 4 where it goes on - and `builds` - by how much ovr_hip_shadow_cache.builds grew over the step (1: the lattice was stale).  They
were written by reading the commit as it was when it was one function of flag assignments; the library of that commit passes the walk unchanged."""
import ctypes as C

import numpy as np

N, SIZE = 24, (96, 64)
INF = float("inf")
MARCHED, CACHED = 0, 1


def _f(values):
    a = np.ascontiguousarray(values, dtype=np.float32).ravel()
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


class Walk:
    def __init__(self, ovr, layout=-1, pipeline=0):
        self.ovr, self.L = ovr, ovr._lib
        self.lib = self.L.load()
        self.base_layout, self.base_pipeline = layout, pipeline
        self.vol = np.ascontiguousarray(ovr.synth.make_volume(N), dtype=np.float32)
        self.tf = {k: ovr.synth.make_tfn(k, 256) for k in ("sparse", "dense")}
        self.cam = ovr.synth.make_camera("oblique", N)
        self.noise = np.ascontiguousarray(ovr.synth.make_noise_tile(16), dtype=np.float32)
        h = C.c_void_p()
        self.L.check(self.lib.ovr_hip_create(C.byref(h), 0))
        self.h = h
        lib, ck = self.lib, self.L.check
        ck(lib.ovr_hip_set_volume_layouts(h, 0))
        ck(lib.ovr_hip_commit(h))  # (the layouts mode is read by the upload)
        ck(lib.ovr_hip_set_fbsize(h, *SIZE))
        ck(lib.ovr_hip_set_frame_accumulation(h, 1))
        ck(lib.ovr_hip_set_shading(h, 2))
        ck(lib.ovr_hip_set_layout_choice(h, layout))
        ck(lib.ovr_hip_set_shading_pipeline(h, pipeline))
        ck(lib.ovr_hip_set_empty_space_skipping(h, 0))
        ck(lib.ovr_hip_set_lds_staging(h, 0))
        self.noise_tile()
        self.tfn("sparse")
        self.camera(0.0)
        self.volume()
        ck(lib.ovr_hip_set_shadow_cache(h, CACHED, 4))
        ck(lib.ovr_hip_commit(h))

    def close(self):
        if self.h:
            self.lib.ovr_hip_destroy(self.h)
            self.h = None

    # ---- the setters, as the C ABI takes them
    def camera(self, shift):
        eye, at, up = self.cam
        self.cam_shift = shift
        _, e = _f((eye[0] + shift, eye[1], eye[2]))
        _, a = _f(at)
        _, u = _f(up)
        self.L.check(self.lib.ovr_hip_set_camera(self.h, e, a, u, 60.0))

    def tfn(self, kind):
        colors, alphas, vr = self.tf[kind]
        c, cp = _f(colors)
        o, op = _f(alphas)
        self.L.check(self.lib.ovr_hip_set_transfer_function(self.h, cp, c.size // 3, op, o.size // 2, float(vr[0]), float(vr[1])))

    def light(self, direction, intensity):
        d = _f(direction)[1] if direction is not None else None
        self.L.check(self.lib.ovr_hip_set_light(self.h, d, float(intensity)))

    def clip(self, on):
        if not on:
            self.L.check(self.lib.ovr_hip_set_clip_box(self.h, None, None))
            return
        self.L.check(self.lib.ovr_hip_set_clip_box(self.h, _f((-INF, -INF, -INF))[1], _f((N / 2.0, INF, INF))[1]))

    def volume(self):
        dims = (C.c_int32 * 3)(N, N, N)
        self.L.check(self.lib.ovr_hip_set_volume(self.h, self.vol.ctypes.data, self.L.MEM_HOST, self.L.TYPE_FLOAT, dims, _f((0, 0, 0))[1], _f((1, 1, 1))[1]))

    def update_volume(self):
        box = np.ascontiguousarray(self.vol[4:12, 4:12, 4:12])
        lo, ext = (C.c_int32 * 3)(4, 4, 4), (C.c_int32 * 3)(8, 8, 8)
        self.L.check(self.lib.ovr_hip_update_volume(self.h, box.ctypes.data, self.L.MEM_HOST, self.L.TYPE_FLOAT, lo, ext))

    def noise_tile(self):
        self.L.check(self.lib.ovr_hip_set_noise_tile(self.h, self.noise.ctypes.data_as(C.POINTER(C.c_float)), 16))

    def call(self, name, *args):
        return lambda: self.L.check(getattr(self.lib, name)(self.h, *args))

    # ---- what the application sees
    def frame_index(self):
        s = self.L.Stats()
        self.L.check(self.lib.ovr_hip_get_stats(self.h, C.byref(s)))
        return s.frame_index

    def builds(self):
        s = self.L.ShadowCache()
        self.L.check(self.lib.ovr_hip_get_shadow_cache(self.h, C.byref(s)))
        return s.builds

    def render(self, frames):
        for _ in range(frames):
            self.L.check(self.lib.ovr_hip_render(self.h))

    def steps(self):
        """(name, apply, index, builds[, prelude]) in the order they run; every source ends on the value it started with"""
        c = self.call
        new_layout = 0 if self.base_layout == -1 else -1
        new_pipeline = 2 if self.base_pipeline != 2 else 1
        R, K = 1, 4  # the accumulation starts over / goes on
        return [
            # ---- the queued values: these reset on ANY call
            ("framebuffer new", c("ovr_hip_set_fbsize", 80, 48), R, 0),
            ("framebuffer same", c("ovr_hip_set_fbsize", 80, 48), R, 0),
            ("framebuffer back", c("ovr_hip_set_fbsize", *SIZE), R, 0),
            ("camera new", lambda: self.camera(3.0), R, 0),
            ("camera same", lambda: self.camera(3.0), R, 0),
            ("camera back", lambda: self.camera(0.0), R, 0),
            ("transfer function new", lambda: self.tfn("dense"), R, 1),
            ("transfer function same", lambda: self.tfn("dense"), R, 1),
            ("transfer function back", lambda: self.tfn("sparse"), R, 1),
            ("grid convention new", c("ovr_hip_set_grid_convention", 1), R, 1),
            ("grid convention same", c("ovr_hip_set_grid_convention", 1), R, 1),
            ("grid convention back", c("ovr_hip_set_grid_convention", 0), R, 1),
            ("focus new", c("ovr_hip_set_focus", 0.5, 0.45, 0.35, 0.15), R, 0),
            ("focus same", c("ovr_hip_set_focus", 0.5, 0.45, 0.35, 0.15), R, 0),
            ("focus back", c("ovr_hip_set_focus", 0.5, 0.5, 0.2, 0.1), R, 0),
            ("spp new", c("ovr_hip_set_sample_per_pixel", 2), R, 0),
            ("spp same", c("ovr_hip_set_sample_per_pixel", 2), R, 0),
            ("spp back", c("ovr_hip_set_sample_per_pixel", 1), R, 0),
            ("sparse sampling new", c("ovr_hip_set_sparse_sampling", 1), R, 0),
            ("sparse sampling same", c("ovr_hip_set_sparse_sampling", 1), R, 0),
            ("sparse sampling back", c("ovr_hip_set_sparse_sampling", 0), R, 0),
            ("accumulation same", c("ovr_hip_set_frame_accumulation", 1), R, 0),
            # without accumulation no frame consumes the reset and the index runs on: 4.  Switching it on again is the next step, with no frames between
            ("accumulation new (off)", c("ovr_hip_set_frame_accumulation", 0), K, 0),
            ("accumulation back", c("ovr_hip_set_frame_accumulation", 1), R, 0, False),
            ("sampling rate new", c("ovr_hip_set_volume_sampling_rate", 2.0), R, 1),
            ("sampling rate same", c("ovr_hip_set_volume_sampling_rate", 2.0), R, 0),  # resets on any call, stale only on another value
            ("sampling rate back", c("ovr_hip_set_volume_sampling_rate", 1.0), R, 1),
            ("shading new", c("ovr_hip_set_shading", 1), R, 0),
            ("shading same", c("ovr_hip_set_shading", 1), R, 0),
            ("shading back", c("ovr_hip_set_shading", 2), R, 0),
            ("jitter new", c("ovr_hip_set_pixel_jitter", 1), R, 0),
            ("jitter same", c("ovr_hip_set_pixel_jitter", 1), R, 0),
            ("jitter back", c("ovr_hip_set_pixel_jitter", 0), R, 0),
            ("convergence new mode", c("ovr_hip_set_convergence", 1, 0.0), R, 0),
            ("convergence same", c("ovr_hip_set_convergence", 1, 0.0), R, 0),
            ("convergence new threshold", c("ovr_hip_set_convergence", 1, 0.5), R, 0),
            ("convergence back", c("ovr_hip_set_convergence", 0, 0.0), R, 0),
            ("reconstruction new", c("ovr_hip_set_reconstruction", 1), R, 0),
            ("reconstruction same", c("ovr_hip_set_reconstruction", 1), R, 0),
            ("reconstruction back", c("ovr_hip_set_reconstruction", 0), R, 0),
            ("image shard new", c("ovr_hip_set_image_shard", 0, 1, 32, 32), R, 0),
            ("image shard same", c("ovr_hip_set_image_shard", 0, 1, 32, 32), R, 0),
            ("image shard back", c("ovr_hip_set_image_shard", 0, 1, 64, 64), R, 0),
            # ---- these only on a CHANGED value
            ("light new direction", lambda: self.light((1.0, 1.0, 1.0), 1.0), R, 1),
            ("light same", lambda: self.light((1.0, 1.0, 1.0), 1.0), K, 0),
            ("light longer vector, same direction", lambda: self.light((2.0, 2.0, 2.0), 1.0), R, 0),
            ("light new intensity", lambda: self.light((2.0, 2.0, 2.0), 1.5), R, 0),
            ("light back", lambda: self.light(None, 1.0), R, 1),
            ("material new", c("ovr_hip_set_material", 0.3, 0.6, 0.4, 12.0), R, 0),
            ("material same", c("ovr_hip_set_material", 0.3, 0.6, 0.4, 12.0), K, 0),
            ("material back", c("ovr_hip_set_material", 0.5, 0.5, 0.0, 0.0), R, 0),
            ("clip box new", lambda: self.clip(True), R, 1),
            ("clip box same", lambda: self.clip(True), K, 0),
            ("clip box back", lambda: self.clip(False), R, 1),
            ("shadow cell new", c("ovr_hip_set_shadow_cache", CACHED, 2), R, 1),
            ("shadow cell same", c("ovr_hip_set_shadow_cache", CACHED, 2), K, 0),
            ("shadow mode new (MARCHED: no lattice is built)", c("ovr_hip_set_shadow_cache", MARCHED, 2), R, 0),
            ("shadow mode same", c("ovr_hip_set_shadow_cache", MARCHED, 2), K, 0),
            ("shadow mode and cell back", c("ovr_hip_set_shadow_cache", CACHED, 4), R, 1),
            # ---- these never: the frame is the same bit for bit
            ("LDS staging new", c("ovr_hip_set_lds_staging", 1), K, 0),
            ("LDS staging same", c("ovr_hip_set_lds_staging", 1), K, 0),
            ("LDS staging back", c("ovr_hip_set_lds_staging", 0), K, 0),
            ("layout choice new", c("ovr_hip_set_layout_choice", new_layout), K, 0),
            ("layout choice same", c("ovr_hip_set_layout_choice", new_layout), K, 0),
            ("layout choice back", c("ovr_hip_set_layout_choice", self.base_layout), K, 0),
            ("pipeline new", c("ovr_hip_set_shading_pipeline", new_pipeline), K, 0),
            ("pipeline same", c("ovr_hip_set_shading_pipeline", new_pipeline), K, 0),
            ("pipeline back", c("ovr_hip_set_shading_pipeline", self.base_pipeline), K, 0),
            ("skipping new", c("ovr_hip_set_empty_space_skipping", 1), K, 0),
            ("skipping same", c("ovr_hip_set_empty_space_skipping", 1), K, 0),
            ("skipping back", c("ovr_hip_set_empty_space_skipping", 0), K, 0),
            # ---- the calls that are no commit (the walk's commit follows them like any other step)
            ("volume upload", self.volume, R, 1),
            ("volume update", self.update_volume, R, 1),
            ("noise tile", self.noise_tile, R, 0),
        ]

    def run(self, report=print):
        """every step; returns the list of (name, index, expected index, builds, expected builds) that missed"""
        bad = []
        for step in self.steps():
            name, apply, index, builds = step[:4]
            if len(step) < 5 or step[4]:
                self.camera(self.cam_shift)
                self.L.check(self.lib.ovr_hip_commit(self.h))
                self.render(3)
                assert self.frame_index() == 3, (name, "the walk's own reset", self.frame_index())
            b0 = self.builds()
            apply()
            self.L.check(self.lib.ovr_hip_commit(self.h))
            self.render(1)
            got, grew = self.frame_index(), self.builds() - b0
            report(f"{name:50s} frame_index {got} (expected {index})   builds +{grew} (expected +{builds})")
            if got != index or grew != builds:
                bad.append((name, got, index, grew, builds))
        return bad
