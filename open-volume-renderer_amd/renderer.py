"""Host-side mirror of the reference's renderer interface for the HIP device.

`DeviceHIP` has the same method names, argument meaning, call protocol and error behaviour as
`ovr::MainRenderer` (reference ovr/renderer.h:82-341) as implemented by its GPU device
(ovr/devices/optix7/device.cpp:16-49): queued thread-safe setters, `init(scene, camera)`, then per frame
`commit()`, `render()`, `mapframe()`, `swap()`.  Everything is forwarded to the C ABI in include/ovr_hip.h;
torch is only used to hand device memory across (volumes living in HBM, frames mapped as tensors)."""
import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from . import lighting

_NP_TO_TYPE = {
    np.dtype(np.uint8): L.TYPE_UINT8, np.dtype(np.int8): L.TYPE_INT8,
    np.dtype(np.uint16): L.TYPE_UINT16, np.dtype(np.int16): L.TYPE_INT16,
    np.dtype(np.uint32): L.TYPE_UINT32, np.dtype(np.int32): L.TYPE_INT32,
    np.dtype(np.float32): L.TYPE_FLOAT, np.dtype(np.float64): L.TYPE_DOUBLE,
}


@dataclass
class Camera:
    """ovr::scene::Camera (reference ovr/scene.h:201-231); fovy defaults to 60 like PerspectiveCamera.  orthographic_height: None = the perspective
    camera; a number = the orthographic camera (scene.h's type ORTHOGRAPHIC) whose image is that high in world units (camera.py), fovy is then not read."""
    eye: Sequence[float] = (0.0, 0.0, -1000.0)   # `from` in the reference (a Python keyword)
    at: Sequence[float] = (0.0, 0.0, 0.0)
    up: Sequence[float] = (0.0, 1.0, 0.0)
    fovy: float = 60.0
    orthographic_height: Optional[float] = None


@dataclass
class TransferFunction:
    """ovr::scene::TransferFunction (scene.h:233-237): color = N x 4 float (rgb + unused w), opacity = M float."""
    color: np.ndarray = None
    opacity: np.ndarray = None
    value_range: Sequence[float] = (1.0, -1.0)


@dataclass
class Scene:
    """The subset of ovr::scene::Scene the path consumes: one structured-regular volume + its transfer function
    (what parse_single_volume_scene accepts, scene.h:413-426) and the render settings main_batch forwards."""
    volume: object = None                      # numpy array or torch tensor, shape (nz, ny, nx), x fastest
    grid_origin: Sequence[float] = (0.0, 0.0, 0.0)
    grid_spacing: Sequence[float] = (1.0, 1.0, 1.0)
    transfer_function: TransferFunction = field(default_factory=TransferFunction)
    camera: Camera = field(default_factory=Camera)
    volume_sampling_rate: float = 1.0
    spp: int = 1
    clipping_box: object = None                # (lower, upper) in world units or None (vidi3d.read_scene: the file's clippingBox)
    slices: Sequence = ()                      # the file's visible cut planes (vidi3d.read_scene) - NOT applied by init: pass them to set_slices


class _DevicePtr:
    """Exposes a raw device pointer through __cuda_array_interface__ so torch.as_tensor can view it without a copy."""

    def __init__(self, ptr, shape, typestr="<f4"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 3}


class CrossDeviceBuffer:
    """Mirror of the reference's CrossDeviceBuffer (ovr/common/cross_device_buffer.h:19-208): a non-owning view of the
    frame, either on the host or on the device; to_cpu() returns host data."""
    DEVICE_CPU, DEVICE_HIP = 0, 1

    def __init__(self):
        self._data = None
        self.device = self.DEVICE_CPU
        self.nbytes = 0

    def set_data(self, data, nbytes, device):
        self._data, self.nbytes, self.device = data, nbytes, device

    def data(self):
        return self._data

    def to_cpu(self):
        if self.device == self.DEVICE_CPU:
            return self
        out = CrossDeviceBuffer()
        out.set_data(self._data.cpu().numpy(), self.nbytes, self.DEVICE_CPU)
        return out


class FrameBufferData:
    """MainRenderer::FrameBufferData (renderer.h:89-97)."""

    def __init__(self):
        self.rgba = CrossDeviceBuffer()
        self.grad = CrossDeviceBuffer()


def _f3(v):
    a = (C.c_float * 3)(*[float(x) for x in v])
    return a


class DeviceHIP:
    """The "hip" device.  Method-for-method mirror of ovr::MainRenderer + DeviceOptix7."""

    def __init__(self, device_id: int = 0, devices=None):
        """devices: several HIP device ordinals -> one in-process device group behind this object (ovr_hip_create_group: image tiles
        sharded over the devices, gathered on devices[0]); the reference's device knows one GPU (device_impl.cpp:371-372)"""
        self._lib = L.load()
        self._h = C.c_void_p()
        if devices is not None and len(devices) > 0:
            ids = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            L.check(self._lib.ovr_hip_create_group(C.byref(self._h), ids, len(devices)))
            device_id = int(devices[0])
        else:
            L.check(self._lib.ovr_hip_create(C.byref(self._h), int(device_id)))
        self.device_id = int(device_id)
        self.current_scene: Optional[Scene] = None
        self.variance = float("inf")          # renderer.h:287
        self._fbsize = (0, 0)
        self._committed_fbsize = (0, 0)       # what the last commit() made current: the size ovr_hip_camera_rays writes
        self._keep = []                        # keeps ctypes buffers alive across calls
        self._convergence_mode = L.CONVERGENCE_OFF
        self._light_dir = None                 # None = the reference's literal
        self._light_angles = lighting.angles_of(lighting.LITERAL_LIGHT)
        self._light_intensity = 1.0
        self._material = lighting.REFERENCE_MATERIAL

    # ---- lifetime -------------------------------------------------------------------------------------------
    def close(self):
        if self._h:
            self._lib.ovr_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- thread-safe setters (renderer.h:135-248) ------------------------------------------------------------
    def set_fbsize(self, fbsize):
        self._fbsize = (int(fbsize[0]), int(fbsize[1]))
        L.check(self._lib.ovr_hip_set_fbsize(self._h, *self._fbsize))

    def set_camera(self, camera_or_from, at=None, up=None):
        """set_camera(Camera) or set_camera(from, at, up).  The three-vector form builds Camera{from, at, up} whose fovy
        is the default 60 degrees - exactly what renderer.h:149-152 does (it discards a scene's fovy)."""
        cam = camera_or_from if isinstance(camera_or_from, Camera) else Camera(camera_or_from, at, up)
        if cam.orthographic_height is not None:
            L.check(self._lib.ovr_hip_set_camera_orthographic(self._h, _f3(cam.eye), _f3(cam.at), _f3(cam.up), float(cam.orthographic_height)))
        else:
            L.check(self._lib.ovr_hip_set_camera(self._h, _f3(cam.eye), _f3(cam.at), _f3(cam.up), float(cam.fovy)))

    def get_camera(self):
        """ovr_hip_get_camera, the COMMITTED camera: kind (0 perspective, 1 orthographic), eye / at / up, fovy, height as given, and pos / dir / hor / ver,
        the basis the kernels read"""
        c = L.CameraState()
        L.check(self._lib.ovr_hip_get_camera(self._h, C.byref(c)))
        return c

    def camera_rays(self, frame_index=1, sample=0):
        """the pixel rays as the kernels form them (ovr_hip_camera_rays; known-answer tests): (org, dir), each (H, W, 3) float32, of the given sample of the
        given frame under the committed camera, framebuffer size, jitter mode and samples per pixel"""
        import torch
        dev = torch.device("cuda", self.device_id)
        w, h = self._committed_fbsize         # (a size queued by set_fbsize and not yet committed is not the entry's)
        out = torch.empty((max(h, 0), max(w, 0), 6), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        L.check(self._lib.ovr_hip_camera_rays(self._h, int(frame_index), int(sample), out.data_ptr(), out.numel()))
        o = out.cpu().numpy()
        return o[..., :3].copy(), o[..., 3:].copy()

    def set_transfer_function(self, c, o, r):
        """c: flat RGB triples, o: flat (position, alpha) pairs, r: (lo, hi) in raw data units (renderer.h:154-161)."""
        c = np.ascontiguousarray(c, dtype=np.float32).ravel()
        o = np.ascontiguousarray(o, dtype=np.float32).ravel()
        if c.size % 3 or o.size % 2:
            raise RuntimeError("transfer function arrays must hold RGB triples and (position, alpha) pairs")
        L.check(self._lib.ovr_hip_set_transfer_function(
            self._h, c.ctypes.data_as(C.POINTER(C.c_float)), c.size // 3, o.ctypes.data_as(C.POINTER(C.c_float)), o.size // 2,
            float(r[0]), float(r[1])))

    def set_focus(self, center, scale, base_noise):
        L.check(self._lib.ovr_hip_set_focus(self._h, float(center[0]), float(center[1]), float(scale), float(base_noise)))

    def set_sample_per_pixel(self, spp):
        L.check(self._lib.ovr_hip_set_sample_per_pixel(self._h, int(spp)))

    def set_sparse_sampling(self, on):
        L.check(self._lib.ovr_hip_set_sparse_sampling(self._h, int(bool(on))))

    def set_frame_accumulation(self, on):
        L.check(self._lib.ovr_hip_set_frame_accumulation(self._h, int(bool(on))))

    def set_volume_sampling_rate(self, rate):
        self._rate_set_by_app = True
        L.check(self._lib.ovr_hip_set_volume_sampling_rate(self._h, float(rate)))

    def set_path_tracing(self, on):
        if on:  # the path tracer is outside this backend's scope
            raise RuntimeError("[hip] path tracing is not part of the ray-marching backend")

    # accepted and ignored, as the reference's ray marcher ignores them (device_impl.cpp:113-197 never reads them): more than one light and the
    # scene file's lights, photon mapping and the density scale belong to its path tracer, and the light's radius - the interactive app has its
    # own call commented out - would make the shadow rays of a frame stop being parallel, which the shade order by light beams relies on
    def set_add_lights(self, v): pass
    def set_photonmapping(self, v): pass
    def set_volume_density_scale(self, v): pass
    def set_light_radius(self, v): pass

    # the seven lighting controls of the interface (renderer.h:210-248), which the reference's OptiX device leaves dead: real here (include/ovr_hip.h,
    # lighting.py).  Angles in degrees, d = (sin phi cos theta, sin phi sin theta, cos phi); the state starts as the reference's literal
    # light and material, setting one value keeps the others.  Queued, applied at commit; a changed value resets the accumulation.
    def set_light_phi(self, v):
        self._push_angles(float(v), self._light_angles[1])

    def set_light_theta(self, v):
        self._push_angles(self._light_angles[0], float(v))

    def _push_angles(self, phi, theta):
        self._push_light(lighting.direction_from_angles(phi, theta))
        self._light_angles = (phi, theta)

    def set_light_intensity(self, v):
        self._push_light(self._light_dir, float(v))

    def set_mat_ambient(self, v): self._push_material(0, v)
    def set_mat_diffuse(self, v): self._push_material(1, v)
    def set_mat_specular(self, v): self._push_material(2, v)
    def set_mat_shininess(self, v): self._push_material(3, v)

    def _push_light(self, direction, intensity=None):
        intensity = self._light_intensity if intensity is None else float(intensity)
        d = None if direction is None else _f3(direction)
        L.check(self._lib.ovr_hip_set_light(self._h, d, intensity))
        # (kept only when the library accepted them)
        self._light_dir, self._light_intensity = None if direction is None else tuple(float(x) for x in direction), intensity

    def _push_material(self, k, v):
        m = list(self._material)
        m[k] = float(v)
        L.check(self._lib.ovr_hip_set_material(self._h, *m))
        self._material = tuple(m)

    def set_light_direction(self, vec, intensity=1.0):
        """direct binding of ovr_hip_set_light: a world-space vector towards the light, any length; None = the reference's literal"""
        self._push_light(None if vec is None else [float(x) for x in vec], intensity)
        self._light_angles = lighting.angles_of(lighting.LITERAL_LIGHT if vec is None else vec)

    def set_material(self, ambient=0.5, diffuse=0.5, specular=0.0, shininess=0.0):
        """direct binding of ovr_hip_set_material; the defaults are the reference's shade expression"""
        m = (float(ambient), float(diffuse), float(specular), float(shininess))
        L.check(self._lib.ovr_hip_set_material(self._h, *m))
        self._material = m

    def lighting(self):
        """ovr_hip_lighting, the COMMITTED state: direction (the unit vector the kernels use), intensity, ambient, diffuse, specular, shininess, is_reference"""
        c = L.Lighting()
        L.check(self._lib.ovr_hip_get_lighting(self._h, C.byref(c)))
        return c

    def shade_floats(self, normal_w, pos, shadow):
        """the shade factor as the kernels evaluate it (ovr_hip_shade_floats; known-answer tests): (n, 3), (n, 3), (n,) -> (n,) float32, with the
        committed light, material and camera position"""
        import torch
        dev = torch.device("cuda", self.device_id)
        t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (normal_w, pos, shadow)]
        n = int(t[2].numel())
        if t[0].numel() != 3 * n or t[1].numel() != 3 * n:
            raise RuntimeError("shade_floats: normal_w and pos hold three floats per sample")
        out = torch.empty(n, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        L.check(self._lib.ovr_hip_shade_floats(self._h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), out.data_ptr(), n))
        return out.cpu().numpy()

    # the clip box (include/ovr_hip.h ovr_hip_set_clip_box; clipping.py is the arithmetic): an axis-aligned box in the space of grid_origin /
    # grid_spacing that cuts the primary rays, the shadow rays and the schedule's block test.  Queued, applied at commit; a changed value resets
    # the accumulation.
    def set_clip_box(self, lower, upper=None):
        """set_clip_box(lower, upper): world coordinates, -inf / +inf = open on that side; set_clip_box(None): no clip box"""
        if lower is None and upper is None:
            L.check(self._lib.ovr_hip_set_clip_box(self._h, None, None))
            return
        lo = None if lower is None else _f3(lower)
        hi = None if upper is None else _f3(upper)
        L.check(self._lib.ovr_hip_set_clip_box(self._h, lo, hi))

    def clip_box(self):
        """ovr_hip_clip_box, the COMMITTED state: enabled, lower / upper (the world box as given), object_lower / object_upper (what the kernels test)"""
        c = L.ClipBox()
        L.check(self._lib.ovr_hip_get_clip_box(self._h, C.byref(c)))
        return c

    def clip_intervals(self, org, direction):
        """the box test as the kernels evaluate it (ovr_hip_clip_intervals; known-answer tests): world rays (n, 3), (n, 3) -> t0 (n,), t1 (n,) float32 and
        hit (n,) bool, with the committed volume and clip box (the unit cube without one)"""
        import torch
        dev = torch.device("cuda", self.device_id)
        t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (org, direction)]
        n = int(t[0].numel()) // 3
        if t[0].numel() != 3 * n or t[1].numel() != 3 * n:
            raise RuntimeError("clip_intervals: org and direction hold three floats per ray")
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        L.check(self._lib.ovr_hip_clip_intervals(self._h, t[0].data_ptr(), t[1].data_ptr(), out.data_ptr(), n))
        o = out.cpu().numpy()
        return o[:, 0].copy(), o[:, 1].copy(), o[:, 2] != 0

    # the shadow cache (include/ovr_hip.h ovr_hip_set_shadow_cache; shadow_cache.py is the arithmetic): the shadow term of full shading from a lattice of the
    # shadow march's values, one trilinear tap per shaded sample.  Queued, applied at commit; a changed mode or cell resets the accumulation.
    def set_shadow_cache(self, mode, cell=0):
        """mode 0 marched (the default), 1 cached, 2 supplied (set_shadow_cache_values first); cell = voxels per lattice cell, 0 = the default"""
        L.check(self._lib.ovr_hip_set_shadow_cache(self._h, int(mode), int(cell)))

    def set_shadow_cache_values(self, array):
        """the lattice of mode 2: a (nz, ny, nx) float32 array of at least 2 nodes per axis spanning the volume; copied at once"""
        a = np.ascontiguousarray(array, dtype=np.float32)
        if a.ndim != 3:
            raise RuntimeError("set_shadow_cache_values: the lattice is a (nz, ny, nx) array")
        dims = (C.c_int32 * 3)(a.shape[2], a.shape[1], a.shape[0])
        L.check(self._lib.ovr_hip_set_shadow_cache_values(self._h, a.ctypes.data, L.MEM_HOST, dims))

    def shadow_cache(self):
        """ovr_hip_shadow_cache, the COMMITTED state: mode, cell, dims, valid, builds, build_shadow_samples, bytes, build_ms"""
        c = L.ShadowCache()
        L.check(self._lib.ovr_hip_get_shadow_cache(self._h, C.byref(c)))
        return c

    def shadow_cache_values(self, member=0, positions=False):
        """the lattice the next cached frame reads as a (nz, ny, nx) float32 array (mode 1 builds it first if it is stale); positions=True: also the nodes'
        world positions, (nz, ny, nx, 3)"""
        dims = (C.c_int32 * 3)()
        L.check(self._lib.ovr_hip_get_shadow_cache_values(self._h, int(member), dims, None, None, 0))
        nx, ny, nz = dims[0], dims[1], dims[2]
        values = np.empty((nz, ny, nx), np.float32)
        pos = np.empty((nz, ny, nx, 3), np.float32) if positions else None
        fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        L.check(self._lib.ovr_hip_get_shadow_cache_values(self._h, int(member), dims, fp(values), fp(pos), values.size))
        return (values, pos) if positions else values

    def shadow_floats(self, pos, which=0):
        """the shadow term as the kernels evaluate it (ovr_hip_shadow_floats; known-answer tests): world positions (n, 3) -> (n,) float32.  which 0: the shadow
        march with the committed light, sampling rate, transfer function and clip box; 1: the lattice lookup"""
        import torch
        dev = torch.device("cuda", self.device_id)
        t = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).to(dev)
        n = int(t.numel()) // 3
        if t.numel() != 3 * n:
            raise RuntimeError("shadow_floats: pos holds three floats per position")
        out = torch.empty(n, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        L.check(self._lib.ovr_hip_shadow_floats(self._h, t.data_ptr(), out.data_ptr(), n, int(which)))
        return out.cpu().numpy()

    # projections (include/ovr_hip.h ovr_hip_set_projection; projection.py is the arithmetic): the maximum, minimum or mean of the samples along each ray in the
    # march's place; the buffer mapframe hands out as `grad` carries the projection layer (v, tm*, 1).  Queued, applied at commit; every call resets the accumulation.
    def set_projection(self, mode):
        """0 off - the march, the default -, 1 maximum, 2 minimum, 3 mean intensity projection (PROJECT_*)"""
        L.check(self._lib.ovr_hip_set_projection(self._h, int(mode)))

    def get_projection(self):
        """ovr_hip_projection, the COMMITTED state: mode, range_skipping (1: the last projection frame ran the range-skipping kernel)"""
        c = L.Projection()
        L.check(self._lib.ovr_hip_get_projection(self._h, C.byref(c)))
        return c

    def project_rays(self, org, direction, mode, range_skipping=False):
        """a projection as the kernels evaluate it (ovr_hip_project_floats; known-answer tests): world rays (n, 3), (n, 3) - the direction used as given - ->
        v (n,), tm* (n,) float32, steps (n,), fetched steps (n,) int64, with the committed volume, sampling rate and clip box; zeros for a ray that is not marched"""
        o = self._ray_query("project_rays", "ovr_hip_project_floats", org, direction, 4, int(mode), int(bool(range_skipping)))
        return o[:, 0].copy(), o[:, 1].copy(), o[:, 2].astype(np.int64), o[:, 3].astype(np.int64)

    def _ray_query(self, what, entry, org, direction, width, *args):
        """the one path of the known-answer ray queries (project_rays ... isosurface_ao_rays): world rays (n, 3), (n, 3) onto the device, the library's `entry`
        called with `args` behind (org, dir, out, n), its records back as (n, width) float32"""
        import torch
        dev = torch.device("cuda", self.device_id)
        t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (org, direction)]
        n = int(t[0].numel()) // 3
        if t[0].numel() != 3 * n or t[1].numel() != 3 * n:
            raise RuntimeError(f"{what}: org and direction hold three floats per ray")
        out = torch.empty((n, width), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        L.check(getattr(self._lib, entry)(self._h, t[0].data_ptr(), t[1].data_ptr(), out.data_ptr(), n, *args))
        return out.cpu().numpy()

    # slices (include/ovr_hip.h ovr_hip_set_slices; slices.py is the arithmetic): up to four cut planes or thick slabs through the volume in the march's place -
    # nearest slice wins; the buffer mapframe hands out as `grad` carries the layer (v, t_k, k + 1).  Queued, applied at commit; every call resets the accumulation.
    def set_slices(self, slices=None):
        """slices: dicts (point, normal, thickness = 0, mode = PROJECT_MAXIMUM) or (point, normal[, thickness[, mode]]) tuples, at most four, kept in the order
        given; thickness 0 a plane, > 0 a slab of that many world units along the normal (inf: the whole box), mode read only for a slab.  None or (): off"""
        items = [] if slices is None else list(slices)
        arr = (L.Slice * max(len(items), 1))()
        for k, s in enumerate(items):
            if isinstance(s, dict):
                point, normal, thickness, mode = s["point"], s["normal"], s.get("thickness", 0.0), s.get("mode", L.PROJECT_MAXIMUM)
            else:
                s = tuple(s)
                point, normal, thickness, mode = s[0], s[1], (s[2] if len(s) > 2 else 0.0), (s[3] if len(s) > 3 else L.PROJECT_MAXIMUM)
            point, normal = np.asarray(point, np.float32).ravel(), np.asarray(normal, np.float32).ravel()
            if point.size != 3 or normal.size != 3:
                raise RuntimeError("set_slices: a point and a normal hold three floats each")
            arr[k].point[:] = [float(x) for x in point]
            arr[k].normal[:] = [float(x) for x in normal]
            arr[k].thickness = float(thickness)
            arr[k].mode = int(mode)
        L.check(self._lib.ovr_hip_set_slices(self._h, arr if items else None, len(items)))

    def slices(self):
        """ovr_hip_slices, the COMMITTED state: n, slice[k].normal / c / thickness / mode, walks (1: a slab is among them), range_skipping (1: the last slice
        frame ran the range-skipping kernel)"""
        c = L.Slices()
        L.check(self._lib.ovr_hip_get_slices(self._h, C.byref(c)))
        return c

    def slice_rays(self, org, direction, range_skipping=False):
        """slice rays as the kernels evaluate them (ovr_hip_slice_floats; known-answer tests): world rays (n, 3), (n, 3) - the direction used as given - ->
        k (n,) int64 - the winning slice's index + 1, 0: nothing met -, v (n,), t_k (n,) float32, steps walked (n,) int64 (a plane: 1), with the committed slices,
        volume, sampling rate and clip box"""
        o = self._ray_query("slice_rays", "ovr_hip_slice_floats", org, direction, 4, int(bool(range_skipping)))
        return o[:, 0].astype(np.int64), o[:, 1].copy(), o[:, 2].copy(), o[:, 3].astype(np.int64)

    # the slice context (include/ovr_hip.h ovr_hip_set_slice_context; slice_context.py is the arithmetic): the unshaded march from the ray's entry up to the winning
    # slice, the opaque slice composited behind it.  Queued, applied at commit; every call resets the accumulation; kept while no slice is committed.
    def set_slice_context(self, mode, opacity_scale=1.0):
        """mode: SLICE_CONTEXT_OFF (0) or SLICE_CONTEXT_FRONT (1); opacity_scale in [0, 1] multiplies every corrected opacity of the context (ignored, and
        stored as 1, in mode OFF).  ValueError where the ABI says EINVAL"""
        code = self._lib.ovr_hip_set_slice_context(self._h, int(mode), float(opacity_scale))
        if code == -1:   # OVR_HIP_EINVAL
            raise ValueError((self._lib.ovr_hip_last_error() or b"").decode("utf-8", "replace"))
        L.check(code)

    def slice_context(self):
        """ovr_hip_slice_context, the COMMITTED state: mode, opacity_scale, active (1: the next frame is a context frame)"""
        c = L.SliceContext()
        L.check(self._lib.ovr_hip_get_slice_context(self._h, C.byref(c)))
        return c

    def slice_context_rays(self, org, direction):
        """context rays as the kernel evaluates them (ovr_hip_slice_context_floats; known-answer tests): world rays (n, 3), (n, 3) - the direction used as given -
        -> k (n,) int64 - the composited slice's index + 1, 0: none -, v (n,), t_k (n,) float32, context steps taken (n,) int64, rgba (n, 4) float32 of the pixel
        sample, with the committed slices, context, transfer function, volume, sampling rate and clip box"""
        o = self._ray_query("slice_context_rays", "ovr_hip_slice_context_floats", org, direction, 8)
        return o[:, 0].astype(np.int64), o[:, 1].copy(), o[:, 2].copy(), o[:, 3].astype(np.int64), o[:, 4:8].copy()

    # pre-integrated classification (include/ovr_hip.h ovr_hip_set_preintegration; preintegration.py is the arithmetic): the unshaded march with every segment
    # between two samples classified by the transfer function's integral over the values it spans.  Queued, applied at commit; every call resets the accumulation;
    # kept, and not drawn, under GRADIENT / FULL shading and while slices, isovalues or a projection are committed.
    def set_preintegration(self, mode):
        """mode: PREINTEGRATION_OFF (0) or PREINTEGRATION_SEGMENTS (1).  ValueError where the ABI says EINVAL"""
        code = self._lib.ovr_hip_set_preintegration(self._h, int(mode))
        if code == -1:   # OVR_HIP_EINVAL
            raise ValueError((self._lib.ovr_hip_last_error() or b"").decode("utf-8", "replace"))
        L.check(code)

    def get_preintegration(self):
        """ovr_hip_preintegration, the COMMITTED state: mode, active (1: the next frame is pre-integrated), nodes and subdivision of the node table built last"""
        c = L.Preintegration()
        L.check(self._lib.ovr_hip_get_preintegration(self._h, C.byref(c)))
        return c

    def preintegration_tables(self):
        """the float32 node table the frames read (ovr_hip_get_preintegration_tables; built if stale): (M, 4) - T, Kr, Kg, Kb per node"""
        n = C.c_int32(0)
        L.check(self._lib.ovr_hip_get_preintegration_tables(self._h, None, 0, C.byref(n)))
        nodes = np.zeros((int(n.value), 4), np.float32)
        L.check(self._lib.ovr_hip_get_preintegration_tables(self._h, nodes.ctypes.data_as(C.POINTER(C.c_float)), int(n.value), C.byref(n)))
        return nodes

    def preintegrated_rays(self, org, direction):
        """pre-integrated rays as the kernel evaluates them (ovr_hip_preintegrated_floats; known-answer tests): world rays (n, 3), (n, 3) - the direction used as
        given - -> segments taken (n,) int64, of them integral-branch segments (n,) int64, tx at exit (n,) float32, rgba (n, 4) float32 of the pixel sample"""
        o = self._ray_query("preintegrated_rays", "ovr_hip_preintegrated_floats", org, direction, 8)
        return o[:, 0].astype(np.int64), o[:, 1].astype(np.int64), o[:, 2].copy(), o[:, 4:8].copy()

    # gradient opacity (include/ovr_hip.h ovr_hip_set_gradient_opacity; gradient_opacity.py is the arithmetic): the march with every sample's table opacity
    # weighted by a ramp over the gradient's magnitude.  Queued, applied at commit; every call resets the accumulation; kept, and not drawn, under FULL shading,
    # while slices, isovalues or a projection are committed, and behind an active pre-integration.
    def set_gradient_opacity(self, mode, lo=0.0, hi=1.0):
        """mode: GRADIENT_OPACITY_OFF (0) or GRADIENT_OPACITY_RAMP (1); lo < hi, finite: the ramp's thresholds in transfer-function ranges per world unit length
        (gradient_opacity.magnitudes gives a volume's).  ValueError where the ABI says EINVAL"""
        code = self._lib.ovr_hip_set_gradient_opacity(self._h, int(mode), float(lo), float(hi))
        if code == -1:   # OVR_HIP_EINVAL
            raise ValueError((self._lib.ovr_hip_last_error() or b"").decode("utf-8", "replace"))
        L.check(code)

    def get_gradient_opacity(self):
        """ovr_hip_gradient_opacity, the COMMITTED state: mode, active (1: the next frame is a gradient-opacity frame), lo, hi, inv_ramp"""
        c = L.GradientOpacity()
        L.check(self._lib.ovr_hip_get_gradient_opacity(self._h, C.byref(c)))
        return c

    def gradient_opacity_rays(self, org, direction, shade=0):
        """gradient-opacity rays as the kernel evaluates them (ovr_hip_gradient_opacity_floats; known-answer tests): world rays (n, 3), (n, 3) - the direction used
        as given - under shading `shade` (0 NONE, 1 GRADIENT) -> steps taken (n,) int64, of them steps that fetched a gradient (n,) int64, tx at exit (n,) float32,
        steps with a > 0 (n,) int64, rgba (n, 4) float32 of the pixel sample"""
        o = self._ray_query("gradient_opacity_rays", "ovr_hip_gradient_opacity_floats", org, direction, 8, int(shade))
        return o[:, 0].astype(np.int64), o[:, 1].astype(np.int64), o[:, 2].copy(), o[:, 3].astype(np.int64), o[:, 4:8].copy()

    # the depth limit (include/ovr_hip.h ovr_hip_set_max_depth; max_depth.py is the arithmetic): the march that ends every ray of a pixel on a ray parameter the
    # caller hands in, so that the frame is what lies in front of the caller's opaque geometry.  Queued, applied at commit; every call resets the accumulation;
    # kept, and not drawn, under FULL shading, while slices, isovalues or a projection are committed, behind an active pre-integration or gradient opacity, and
    # while the image's size is not the committed framebuffer's.
    def set_max_depth(self, depth=None, size=None):
        """depth: a (height, width) float32 array in the frame's pixel order - the order of mapframe's rgba - or a flat one with size = (width, height); None
        switches the limit off.  UNITS: the march's t - world length along the normalised ray direction from the ray's origin: under the perspective camera the
        Euclidean distance from the camera position (not a planar z, not a z-buffer value; max_depth.ray_distance_from_planar converts one), under the
        orthographic camera the distance from the image plane through `from`.  +inf or NaN: no surface at that pixel.  Copied at once.  ValueError where the
        ABI says EINVAL"""
        if depth is None:
            L.check(self._lib.ovr_hip_set_max_depth(self._h, None, L.MEM_HOST, 0, 0))
            return
        a = np.ascontiguousarray(depth, dtype=np.float32)
        if size is None:
            if a.ndim != 2:
                raise RuntimeError("set_max_depth: the image is a (height, width) array, or a flat one with size = (width, height)")
            w, h = a.shape[1], a.shape[0]
        else:
            w, h = int(size[0]), int(size[1])
            if w >= 1 and h >= 1 and w * h <= 2 ** 31 - 1 and a.size != w * h:      # (a size the ABI refuses is refused there, before the image is read)
                raise RuntimeError("set_max_depth: the image holds width * height values")
        code = self._lib.ovr_hip_set_max_depth(self._h, a.ctypes.data, L.MEM_HOST, int(w), int(h))
        if code == -1:   # OVR_HIP_EINVAL
            raise ValueError((self._lib.ovr_hip_last_error() or b"").decode("utf-8", "replace"))
        L.check(code)

    def get_max_depth(self, values=False):
        """ovr_hip_max_depth, the COMMITTED state: mode, active (1: the next frame is a depth-limited frame), width, height; values=True: (state, the committed
        image as a (height, width) float32 array, None in mode OFF)"""
        c = L.MaxDepth()
        L.check(self._lib.ovr_hip_get_max_depth(self._h, C.byref(c)))
        if not values:
            return c
        w, h = C.c_int32(0), C.c_int32(0)
        L.check(self._lib.ovr_hip_get_max_depth_values(self._h, None, 0, C.byref(w), C.byref(h)))
        if w.value < 1 or h.value < 1:
            return c, None
        out = np.empty((h.value, w.value), np.float32)
        L.check(self._lib.ovr_hip_get_max_depth_values(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(w), C.byref(h)))
        return c, out

    def max_depth_rays(self, org, direction, depth, shade=0):
        """depth-limited rays as the kernel evaluates them (ovr_hip_max_depth_floats; known-answer tests): world rays (n, 3), (n, 3) - the direction used as
        given - ray i ending on depth[i] (n,), under shading `shade` (0 NONE, 1 GRADIENT) -> steps taken (n,) int64, the cut tc (n,) float32, tx at exit (n,)
        float32, steps with a > 0 (n,) int64, rgba (n, 4) float32 of the pixel sample"""
        import torch
        dev = torch.device("cuda", self.device_id)
        t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (org, direction, depth)]
        n = int(t[0].numel()) // 3
        if t[0].numel() != 3 * n or t[1].numel() != 3 * n or t[2].numel() != n:
            raise RuntimeError("max_depth_rays: org and direction hold three floats per ray, depth one")
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        code = self._lib.ovr_hip_max_depth_floats(self._h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), out.data_ptr(), n, int(shade))
        if code == -1:   # OVR_HIP_EINVAL
            raise ValueError((self._lib.ovr_hip_last_error() or b"").decode("utf-8", "replace"))
        L.check(code)
        o = out.cpu().numpy()
        return o[:, 0].astype(np.int64), o[:, 1].copy(), o[:, 2].copy(), o[:, 3].astype(np.int64), o[:, 4:8].copy()

    # the depth layer (include/ovr_hip.h ovr_hip_set_depth_output; depth_output.py is the arithmetic): the march that also writes where along each ray it became
    # opaque into the buffer mapframe hands out as `grad` - (d, S, reached); depth_output.resolve turns a frame into depths.  Queued, applied at commit; every
    # call resets the accumulation; kept, and not drawn, under FULL shading, while slices, isovalues or a projection are committed, and behind an active
    # pre-integration or gradient opacity.
    def set_depth_output(self, threshold=None):
        """threshold: tau in (0, 0.9999] - the accumulated opacity at which a ray counts as having reached its surface (the smallest positive normal float:
        the first step with opacity; 0.5: the median surface); None switches the output off.  ValueError where the ABI says EINVAL"""
        if threshold is None:
            L.check(self._lib.ovr_hip_set_depth_output(self._h, L.DEPTH_OUTPUT_OFF, 0.0))
            return
        code = self._lib.ovr_hip_set_depth_output(self._h, L.DEPTH_OUTPUT_ON, float(threshold))
        if code == -1:   # OVR_HIP_EINVAL
            raise ValueError((self._lib.ovr_hip_last_error() or b"").decode("utf-8", "replace"))
        L.check(code)

    def get_depth_output(self):
        """ovr_hip_depth_output, the COMMITTED state: mode, active (1: the next frame is a depth frame), limited (1: it applies the committed depth image),
        threshold"""
        c = L.DepthOutput()
        L.check(self._lib.ovr_hip_get_depth_output(self._h, C.byref(c)))
        return c

    def depth_output_rays(self, org, direction, threshold, depth=None, shade=0):
        """depth-output rays as the kernel evaluates them (ovr_hip_depth_output_floats; known-answer tests): world rays (n, 3), (n, 3) - the direction used as
        given - ray i ending on depth[i] (n,) (None: no limit on any ray), under shading `shade` (0 NONE, 1 GRADIENT) -> dict(steps (n,) int64, tc, tx (n,)
        float32, shaded (n,) int64, rgba (n, 4) float32, reached (n,) bool, d (n,) float32, k (n,) int64, S (n,) float32)"""
        import torch
        dev = torch.device("cuda", self.device_id)
        arrays = (org, direction) if depth is None else (org, direction, depth)
        t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in arrays]
        n = int(t[0].numel()) // 3
        if t[0].numel() != 3 * n or t[1].numel() != 3 * n or (depth is not None and t[2].numel() != n):
            raise RuntimeError("depth_output_rays: org and direction hold three floats per ray, depth one")
        out = torch.empty((n, 12), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        code = self._lib.ovr_hip_depth_output_floats(self._h, t[0].data_ptr(), t[1].data_ptr(), None if depth is None else t[2].data_ptr(), out.data_ptr(), n, int(shade), float(threshold))
        if code == -1:   # OVR_HIP_EINVAL
            raise ValueError((self._lib.ovr_hip_last_error() or b"").decode("utf-8", "replace"))
        L.check(code)
        o = out.cpu().numpy()
        return dict(steps=o[:, 0].astype(np.int64), tc=o[:, 1].copy(), tx=o[:, 2].copy(), shaded=o[:, 3].astype(np.int64), rgba=o[:, 4:8].copy(),
                    reached=o[:, 8] != 0, d=o[:, 9].copy(), k=o[:, 10].astype(np.int64), S=o[:, 11].copy())

    # isosurfaces (include/ovr_hip.h ovr_hip_set_isosurfaces; isosurface.py is the arithmetic): opaque, shaded, hard-shadowed level sets in the march's place; the
    # buffer mapframe hands out as `grad` carries the layer (isovalue, t*, 1).  Queued, applied at commit; every call resets the accumulation.
    def set_isosurfaces(self, values=(), opacities=None):
        """up to four finite, distinct isovalues in the samples' units (8-bit types normalised); none: off, the default.  opacities (one per isovalue, in (0, 1],
        ovr_hip_set_isosurface_layers): with one below 1 the level sets are translucent - every crossing of a ray composited front to back; None: opaque"""
        v = np.ascontiguousarray(values, dtype=np.float32).ravel()
        pv = v.ctypes.data_as(C.POINTER(C.c_float)) if v.size else None
        if opacities is None:
            L.check(self._lib.ovr_hip_set_isosurfaces(self._h, pv, int(v.size)))
            return
        a = np.ascontiguousarray(opacities, dtype=np.float32).ravel()
        if a.size != v.size:
            raise RuntimeError("set_isosurfaces: one opacity per isovalue")
        L.check(self._lib.ovr_hip_set_isosurface_layers(self._h, pv, a.ctypes.data_as(C.POINTER(C.c_float)) if a.size else None, int(v.size)))

    def get_isosurface_layers(self):
        """ovr_hip_isosurface_layers, the COMMITTED state: n, isovalues (ascending), opacities, translucent (1: a committed opacity is below 1), range_skipping"""
        c = L.IsosurfaceLayers()
        L.check(self._lib.ovr_hip_get_isosurface_layers(self._h, C.byref(c)))
        return c

    def isosurface_layer_rays(self, org, direction, max_events=8, range_skipping=False):
        """translucent isosurface rays as the kernels evaluate them (ovr_hip_isosurface_layers_floats; known-answer tests): world rays (n, 3), (n, 3) ->
        dict(events (n,) int64 - composited -, A (n,) float32, steps, shadow_steps (n,) int64, and per event slot e < max_events k (n, e) int64, t, shadow,
        A_after (n, e) float32, normal (n, e, 3); zeros behind a ray's events) with the committed isovalues, opacities, volume, sampling rate, light and clip box"""
        m = int(max_events)
        o = self._ray_query("isosurface_layer_rays", "ovr_hip_isosurface_layers_floats", org, direction, 4 + 8 * max(m, 0), m, int(bool(range_skipping)))
        e = o[:, 4:].reshape(len(o), m, 8)
        return dict(events=o[:, 0].astype(np.int64), A=o[:, 1].copy(), steps=o[:, 2].astype(np.int64), shadow_steps=o[:, 3].astype(np.int64), k=e[:, :, 0].astype(np.int64),
                    t=e[:, :, 1].copy(), normal=e[:, :, 2:5].copy(), shadow=e[:, :, 5].copy(), A_after=e[:, :, 6].copy())

    # the isosurface context (include/ovr_hip.h ovr_hip_set_isosurface_context; isosurface_context.py is the arithmetic): the unshaded march composited around
    # the level sets' events, one walk for both.  Queued, applied at commit; every call resets the accumulation; kept while no isovalue is committed.
    def set_isosurface_context(self, mode, opacity_scale=1.0):
        """mode: ISO_CONTEXT_OFF (0) or ISO_CONTEXT_VOLUME (1); opacity_scale in [0, 1] multiplies every corrected opacity of the volume (ignored, and stored as
        1, in mode OFF; the isovalues' own opacities are not touched).  ValueError where the ABI says EINVAL"""
        code = self._lib.ovr_hip_set_isosurface_context(self._h, int(mode), float(opacity_scale))
        if code == -1:   # OVR_HIP_EINVAL
            raise ValueError((self._lib.ovr_hip_last_error() or b"").decode("utf-8", "replace"))
        L.check(code)

    def get_isosurface_context(self):
        """ovr_hip_isosurface_context, the COMMITTED state: mode, opacity_scale, active (1: the next frame is a context frame)"""
        c = L.IsosurfaceContext()
        L.check(self._lib.ovr_hip_get_isosurface_context(self._h, C.byref(c)))
        return c

    def isosurface_context_rays(self, org, direction, max_events=8):
        """context rays as the kernel evaluates them (ovr_hip_isosurface_context_floats; known-answer tests), under full shading: world rays (n, 3), (n, 3) ->
        dict(events (n,) int64 - composited -, A (n,) float32, steps, shadow_steps, lit (n,) int64 - volume samples with a' > 0 -, rgb (n, 3) float32 of the pixel
        sample, and per event slot e < max_events k (n, e) int64, t, shadow, A_after (n, e) float32, normal (n, e, 3); zeros behind a ray's events) with the
        committed isovalues, opacities, context, transfer function, volume, sampling rate, light, material and clip box"""
        m = int(max_events)
        o = self._ray_query("isosurface_context_rays", "ovr_hip_isosurface_context_floats", org, direction, 8 + 8 * max(m, 0), m)
        e = o[:, 8:].reshape(len(o), m, 8)
        return dict(events=o[:, 0].astype(np.int64), A=o[:, 1].copy(), steps=o[:, 2].astype(np.int64), shadow_steps=o[:, 3].astype(np.int64), rgb=o[:, 4:7].copy(),
                    lit=o[:, 7].astype(np.int64), k=e[:, :, 0].astype(np.int64), t=e[:, :, 1].copy(), normal=e[:, :, 2:5].copy(), shadow=e[:, :, 5].copy(),
                    A_after=e[:, :, 6].copy())

    # ambient occlusion of the isosurface frames (include/ovr_hip.h ovr_hip_set_ambient_occlusion; isosurface.py is the arithmetic).  Queued, applied at commit;
    # every call resets the accumulation.
    def set_ambient_occlusion(self, samples, distance=float("inf")):
        """samples = K in 0 ... 16 occlusion walks per event of a GRADIENT- or FULL-shaded isosurface frame, each at most `distance` long (world units; inf: the
        whole box); 0: off, the default"""
        L.check(self._lib.ovr_hip_set_ambient_occlusion(self._h, int(samples), float(distance)))

    def get_ambient_occlusion(self):
        """ovr_hip_ambient_occlusion, the COMMITTED state: samples, distance, rotations (16), active (1: the next isosurface frame takes the AO kernels)"""
        c = L.AmbientOcclusion()
        L.check(self._lib.ovr_hip_get_ambient_occlusion(self._h, C.byref(c)))
        return c

    def ambient_occlusion_directions(self):
        """the COMMITTED direction table as the host formed it: (16, K, 3) float32"""
        k = int(self.get_ambient_occlusion().samples)
        out = np.zeros((L.AO_ROTATIONS, k, 3), np.float32)
        buf = (C.c_float * max(out.size, 1))()
        L.check(self._lib.ovr_hip_get_ambient_occlusion_directions(self._h, buf, out.size))
        if out.size:
            out[...] = np.frombuffer(buf, np.float32, out.size).reshape(out.shape)
        return out

    def isosurface_ao_rays(self, org, direction, rotation=0, max_events=8, range_skipping=False):
        """isosurface rays with ambient occlusion as the kernels evaluate them (ovr_hip_isosurface_ao_floats; known-answer tests): world rays (n, 3), (n, 3), every
        ray at the rotation `rotation` of the direction table -> isosurface_layer_rays' dict plus O (n, e) float32 per event slot and ao_steps, ao_fetched (n,)
        int64: the steps the AO walks of all events walked and fetched"""
        m = int(max_events)
        o = self._ray_query("isosurface_ao_rays", "ovr_hip_isosurface_ao_floats", org, direction, 8 + 8 * max(m, 0), m, int(rotation), int(bool(range_skipping)))
        e = o[:, 8:].reshape(len(o), m, 8)
        return dict(events=o[:, 0].astype(np.int64), A=o[:, 1].copy(), steps=o[:, 2].astype(np.int64), shadow_steps=o[:, 3].astype(np.int64),
                    ao_steps=o[:, 4].astype(np.int64), ao_fetched=o[:, 5].astype(np.int64), k=e[:, :, 0].astype(np.int64), t=e[:, :, 1].copy(),
                    normal=e[:, :, 2:5].copy(), shadow=e[:, :, 5].copy(), A_after=e[:, :, 6].copy(), O=e[:, :, 7].copy())

    def get_isosurfaces(self):
        """ovr_hip_isosurfaces, the COMMITTED state: n, isovalues (ascending), range_skipping (1: the last isosurface frame ran the range-skipping kernel)"""
        c = L.Isosurfaces()
        L.check(self._lib.ovr_hip_get_isosurfaces(self._h, C.byref(c)))
        return c

    def isosurface_rays(self, org, direction, range_skipping=False):
        """isosurface rays as the kernels evaluate them (ovr_hip_isosurface_floats; known-answer tests): world rays (n, 3), (n, 3) - the direction used as given - ->
        dict(hit (n,) bool, iso, t (n,) float32, steps (n,) int64, normal (n, 3), shadow (n,)) with the committed isovalues, volume, sampling rate, light and clip box"""
        o = self._ray_query("isosurface_rays", "ovr_hip_isosurface_floats", org, direction, 8, int(bool(range_skipping)))
        return dict(hit=o[:, 0] != 0, iso=o[:, 1].copy(), t=o[:, 2].copy(), steps=o[:, 3].astype(np.int64), normal=o[:, 4:7].copy(), shadow=o[:, 7].copy())

    # ---- extensions of this backend ----------------------------------------------------------------------------
    def set_shading(self, mode):
        L.check(self._lib.ovr_hip_set_shading(self._h, int(mode)))

    def set_shading_pipeline(self, mode):
        """0 auto, 1 in place, 2 pooled (include/ovr_hip.h) - both produce bit-identical frames"""
        L.check(self._lib.ovr_hip_set_shading_pipeline(self._h, int(mode)))

    def set_empty_space_skipping(self, on):
        """skip the voxel fetch of samples in macrocells whose max TF opacity is 0 (frames stay bit-identical)"""
        L.check(self._lib.ovr_hip_set_empty_space_skipping(self._h, int(bool(on))))

    def macrocells(self):
        """(minmax[mz,my,mx,2], majorant[mz,my,mx]) of the reference's 16^3 macrocell grids"""
        dims = (C.c_int32 * 3)()
        L.check(self._lib.ovr_hip_get_macrocells(self._h, dims, None, None, 0))
        n = dims[0] * dims[1] * dims[2]
        mm = np.zeros((dims[2], dims[1], dims[0], 2), np.float32)
        mj = np.zeros((dims[2], dims[1], dims[0]), np.float32)
        L.check(self._lib.ovr_hip_get_macrocells(self._h, dims, mm.ctypes.data_as(C.POINTER(C.c_float)), mj.ctypes.data_as(C.POINTER(C.c_float)), n))
        return mm, mj

    def set_pixel_jitter(self, mode):
        """0 = RandomTEA, applied iff spp > 1 (the reference); 1 = blue-noise tile (set_noise_tile), applied to every sample
        of every frame - progressive accumulation with frame-indexed slices (BASELINE C5)"""
        L.check(self._lib.ovr_hip_set_pixel_jitter(self._h, int(mode)))

    def volume_info(self):
        """dims, bytes resident in HBM, the data range found at load (array.cpp:27-66,297) and the TF range in effect"""
        v = L.VolumeInfo()
        L.check(self._lib.ovr_hip_get_volume_info(self._h, C.byref(v)))
        return v

    def set_lds_staging(self, on):
        """LDS-staged bricks for the unshaded march of float volumes (include/ovr_hip.h); off by default"""
        L.check(self._lib.ovr_hip_set_lds_staging(self._h, int(bool(on))))

    def set_phase_timing(self, on):
        """per-phase device times in stats() (march_ms / shade_ms / composite_ms): on by default; off saves the two events between the
        frame's kernels (~16 us per frame).  kernel_ms is measured either way; frames are identical."""
        L.check(self._lib.ovr_hip_set_phase_timing(self._h, int(bool(on))))

    def set_volume_layouts(self, mode):
        """which layouts of the volume the next init / volume upload keeps in HBM: 0 general only, 1 (default) thin replicas
        when they fit comfortably, 2 always (include/ovr_hip.h)"""
        L.check(self._lib.ovr_hip_set_volume_layouts(self._h, int(mode)))

    def set_layout_choice(self, choice):
        """-1 (default): automatic (camera direction; the quad replica for frames that shade every sample); 0 / 1 / 2 / 3: forced
        (general, thin, thin transposed, quad).  Frames are bit-identical."""
        L.check(self._lib.ovr_hip_set_layout_choice(self._h, int(choice)))

    def set_convergence(self, mode, threshold=0.0):
        """convergence estimate (include/ovr_hip.h, convergence.py): 0 off, 1 estimate - frames unchanged, render() stores the frame error in
        `variance` -, 2 adaptive - 8x8 blocks whose error is <= threshold are retired: no longer marched, shown as their mean.  Applied at commit;
        resets the accumulation."""
        L.check(self._lib.ovr_hip_set_convergence(self._h, int(mode), float(threshold)))
        self._convergence_mode = int(mode)

    def convergence(self):
        """ovr_hip_convergence of the last frame: error (inf while valid == 0), threshold, mode, valid, frames, blocks, active_blocks, retired_blocks"""
        c = L.Convergence()
        L.check(self._lib.ovr_hip_get_convergence(self._h, C.byref(c)))
        return c

    def convergence_blocks(self, member=0):
        """(E_b[by, bx] float32, n_b[by, bx] int32 - negative when the block is retired) of one member (known-answer tests)"""
        dims = (C.c_int32 * 2)()
        L.check(self._lib.ovr_hip_get_convergence_blocks(self._h, int(member), dims, None, None, 0))
        err = np.zeros((dims[1], dims[0]), np.float32)
        frames = np.zeros((dims[1], dims[0]), np.int32)
        L.check(self._lib.ovr_hip_get_convergence_blocks(self._h, int(member), dims, err.ctypes.data_as(C.POINTER(C.c_float)),
                                                         frames.ctypes.data_as(C.POINTER(C.c_int32)), err.size))
        return err, frames

    def accumulation(self, which=0, member=0):
        """the accumulation buffer A (which = 0) or H, the sum of the even-numbered frames (1), as (H, W, 4) float32 (known-answer tests)"""
        w, h = self._fbsize
        out = np.zeros((h, w, 4), np.float32)
        L.check(self._lib.ovr_hip_get_accumulation(self._h, int(member), int(which), out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def set_reconstruction(self, mode):
        """pull-push hole filling of sparse-sampled frames (include/ovr_hip.h, reconstruction.py): 0 off, 1 fill - a frame rendered with sparse
        sampling on is completed on the device before anything maps it; dense frames are unchanged.  Applied at commit; resets the accumulation."""
        L.check(self._lib.ovr_hip_set_reconstruction(self._h, int(mode)))

    def reconstruction(self):
        """ovr_hip_reconstruction of the last frame: mode, valid, levels, sampled_pixels, filled_pixels, reconstruct_ms"""
        c = L.Reconstruction()
        L.check(self._lib.ovr_hip_get_reconstruction(self._h, C.byref(c)))
        return c

    def reconstruction_weights(self):
        """N as (H, W) float32: how many frames of the running accumulation (this frame alone without accumulation) sampled each pixel"""
        w, h = self._fbsize
        out = np.zeros((h, w), np.float32)
        L.check(self._lib.ovr_hip_get_reconstruction_weights(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def reconstruction_gradient(self):
        """G as (H, W, 3) float32: the gradient layer of the sampled pixels, accumulated like A (accumulating frames only)"""
        w, h = self._fbsize
        out = np.zeros((h, w, 3), np.float32)
        L.check(self._lib.ovr_hip_get_reconstruction_gradient(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def reconstruct_image(self, rgba, grad, weight):
        """fills the holes of a device image in place with the renderer's kernels: rgba (H, W, 4), grad (H, W, 3) or None, weight (H, W) - > 0 = sampled,
        not modified -, contiguous float32 torch tensors on this renderer's device.  Returns (rgba, grad)."""
        import torch
        dev = torch.device("cuda", self.device_id)
        for name, t, last in (("rgba", rgba, 4), ("grad", grad, 3), ("weight", weight, None)):
            if t is None and name == "grad":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise RuntimeError(f"reconstruct_image: {name} must be a contiguous float32 tensor on {dev}")
            if last is not None and (t.dim() != 3 or t.shape[2] != last):
                raise RuntimeError(f"reconstruct_image: {name} must have shape (H, W, {last})")
        h, w = int(rgba.shape[0]), int(rgba.shape[1])
        if tuple(weight.shape) != (h, w) or (grad is not None and tuple(grad.shape[:2]) != (h, w)):
            raise RuntimeError("reconstruct_image: the planes disagree on the image size")
        torch.cuda.current_stream(dev).synchronize()  # the kernels run on the renderer's stream
        L.check(self._lib.ovr_hip_reconstruct_image(self._h, rgba.data_ptr(), grad.data_ptr() if grad is not None else None, weight.data_ptr(), w, h))
        return rgba, grad

    def set_grid_convention(self, convention):
        L.check(self._lib.ovr_hip_set_grid_convention(self._h, int(convention)))

    def set_noise_tile(self, tile):
        tile = np.ascontiguousarray(tile, dtype=np.float32)
        xy = int(round((tile.size // 64) ** 0.5))
        if xy * xy * 64 != tile.size:
            raise RuntimeError("noise tile must hold xy*xy*64 floats, layout [y][x][t]")
        L.check(self._lib.ovr_hip_set_noise_tile(self._h, tile.ctypes.data_as(C.POINTER(C.c_float)), xy))

    def set_image_shard(self, rank, world, tile_w=64, tile_h=64):
        L.check(self._lib.ovr_hip_set_image_shard(self._h, int(rank), int(world), int(tile_w), int(tile_h)))

    def set_stream(self, stream_ptr):
        L.check(self._lib.ovr_hip_set_stream(self._h, C.c_void_p(int(stream_ptr) if stream_ptr else None)))

    # ---- init / per-frame protocol (renderer.h:107-116,290-341) ----------------------------------------------
    def set_scene(self, scene: Scene):
        """MainRenderer::set_scene (renderer.h:299-341): flatten the scene TF into the app-side format and queue it."""
        tfn = scene.transfer_function
        if tfn is not None and tfn.color is not None and tfn.opacity is not None:
            color = np.asarray(tfn.color, dtype=np.float32).reshape(-1, 4)
            opacity = np.asarray(tfn.opacity, dtype=np.float32).ravel()
            tfn_colors = color[:, :3].ravel()
            pos = np.arange(opacity.size, dtype=np.float32) / np.float32(max(opacity.size - 1, 1))
            tfn_alphas = np.stack([pos, opacity], axis=1).ravel()
            self.set_transfer_function(tfn_colors, tfn_alphas, tfn.value_range)
        self.current_scene = scene

    def init(self, scene: Scene, camera: Camera):
        """MainRenderer::init(argc, argv, scene, camera) (renderer.h:290-297) followed by DeviceOptix7::init ->
        Impl::buildScene (device_impl.cpp:283-302): upload the volume, take the scene's sampling rate, first commit."""
        self.set_scene(scene)
        self.set_camera(camera)
        self._upload_volume(scene)
        if scene.clipping_box is not None:
            self.set_clip_box(*scene.clipping_box)
        # buildScene applies the scene's rate directly; an earlier set_volume_sampling_rate() stays queued and wins at commit
        # (device_impl.cpp:298 then :190-196) - reproduced by not queuing the scene's rate when the app already set one.
        if not getattr(self, "_rate_set_by_app", False):
            L.check(self._lib.ovr_hip_set_volume_sampling_rate(self._h, float(scene.volume_sampling_rate)))
        self.commit()

    @staticmethod
    def _volume_array(vol):
        """a (nz, ny, nx) numpy array or torch tensor, host or device -> (contiguous array - keep it alive -, pointer, mem kind, value type)"""
        if isinstance(vol, np.ndarray):
            if vol.ndim != 3:
                raise RuntimeError("volume must have shape (nz, ny, nx)")
            vol = np.ascontiguousarray(vol)
            vt = _NP_TO_TYPE.get(vol.dtype)
            if vt is None:
                raise RuntimeError("[Optix7] unexpected volume type ...")
            return vol, C.c_void_p(vol.ctypes.data), L.MEM_HOST, vt
        import torch
        if not isinstance(vol, torch.Tensor) or vol.dim() != 3:
            raise RuntimeError("volume must be a numpy array or torch tensor of shape (nz, ny, nx)")
        vol = vol.contiguous()
        tmap = {torch.uint8: L.TYPE_UINT8, torch.int8: L.TYPE_INT8, torch.int16: L.TYPE_INT16, torch.int32: L.TYPE_INT32,
                torch.float32: L.TYPE_FLOAT, torch.float64: L.TYPE_DOUBLE}
        if hasattr(torch, "uint16"):
            tmap[torch.uint16] = L.TYPE_UINT16
        vt = tmap.get(vol.dtype)
        if vt is None:
            raise RuntimeError("[Optix7] unexpected volume type ...")
        if vol.is_cuda:
            torch.cuda.current_stream(vol.device).synchronize()
        return vol, C.c_void_p(vol.data_ptr()), (L.MEM_DEVICE if vol.is_cuda else L.MEM_HOST), vt

    def _upload_volume(self, scene: Scene):
        if scene.volume is None:
            raise RuntimeError("expect only one instance")  # parse_single_volume_scene, scene.h:416
        origin, spacing = _f3(scene.grid_origin), _f3(scene.grid_spacing)
        vol, ptr, kind, vt = self._volume_array(scene.volume)
        dims = (C.c_int32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
        L.check(self._lib.ovr_hip_set_volume(self._h, ptr, kind, vt, dims, origin, spacing))

    def update_volume(self, array, lower):
        """ovr_hip_update_volume: `array` (nz, ny, nx) - numpy or torch, host or device, of the resident volume's type -
        replaces the voxels [lower, lower + extent) of the resident volume in place; lower = (x, y, z).  Immediate, like the upload in init();
        afterwards the renderer is, bit for bit, what a fresh upload of the patched array would have made it."""
        vol, ptr, kind, vt = self._volume_array(array)
        lo = (C.c_int32 * 3)(*[int(v) for v in lower])
        ext = (C.c_int32 * 3)(vol.shape[2], vol.shape[1], vol.shape[0])
        L.check(self._lib.ovr_hip_update_volume(self._h, ptr, kind, vt, lo, ext))

    def update_times(self):
        """milliseconds of the last update_volume: dict(total, alloc, copy, kernels), like upload_times()"""
        out = (C.c_double * 4)()
        L.check(self._lib.ovr_hip_get_update_times(self._h, out))
        return dict(total_ms=out[0], alloc_ms=out[1], copy_ms=out[2], kernels_ms=out[3])

    def volume_layout(self, layout, member=0):
        """the raw bytes (numpy uint8) of a resident layout of the volume, 0 general ... 3 quad: a known-answer hook like macrocells()"""
        n = C.c_uint64()
        L.check(self._lib.ovr_hip_get_volume_layout(self._h, int(member), int(layout), None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint8)
        L.check(self._lib.ovr_hip_get_volume_layout(self._h, int(member), int(layout), C.c_void_p(out.ctypes.data), out.nbytes, C.byref(n)))
        return out

    def commit(self):
        L.check(self._lib.ovr_hip_commit(self._h))
        self._committed_fbsize = self._fbsize

    def render(self):
        L.check(self._lib.ovr_hip_render(self._h))
        self.variance = 0.0  # device_impl.cpp:266
        if self._convergence_mode != L.CONVERGENCE_OFF:  # the frame error, as the reference's OSPRay device fills it in (renderer.h:124-127)
            c = self.convergence()
            self.variance = float(c.error) if c.valid else float("inf")

    def render_async(self):
        L.check(self._lib.ovr_hip_render_async(self._h))

    def sync(self):
        L.check(self._lib.ovr_hip_sync(self._h))

    def swap(self):
        L.check(self._lib.ovr_hip_swap(self._h))

    def mapframe(self, fb: FrameBufferData, device: bool = False):
        """Impl::mapframe (device_impl.cpp:271-281).  device=True hands out device memory as torch tensors (what the
        reference does, DEVICE_CUDA); device=False returns host arrays (the caller's to_cpu())."""
        rgba, grad = C.c_void_p(), C.c_void_p()
        nb_rgba, nb_grad = C.c_size_t(), C.c_size_t()
        kind = L.MEM_DEVICE if device else L.MEM_HOST
        L.check(self._lib.ovr_hip_mapframe(self._h, kind, C.byref(rgba), C.byref(nb_rgba), C.byref(grad), C.byref(nb_grad)))
        w, h = self._fbsize
        if device:
            import torch
            dev = torch.device("cuda", self.device_id)
            t_rgba = torch.as_tensor(_DevicePtr(rgba.value, (h, w, 4)), device=dev)
            t_grad = torch.as_tensor(_DevicePtr(grad.value, (h, w, 3)), device=dev)
            fb.rgba.set_data(t_rgba, nb_rgba.value, CrossDeviceBuffer.DEVICE_HIP)
            fb.grad.set_data(t_grad, nb_grad.value, CrossDeviceBuffer.DEVICE_HIP)
        else:
            a_rgba = np.ctypeslib.as_array(C.cast(rgba, C.POINTER(C.c_float)), shape=(h, w, 4))
            a_grad = np.ctypeslib.as_array(C.cast(grad, C.POINTER(C.c_float)), shape=(h, w, 3))
            fb.rgba.set_data(a_rgba, nb_rgba.value, CrossDeviceBuffer.DEVICE_CPU)
            fb.grad.set_data(a_grad, nb_grad.value, CrossDeviceBuffer.DEVICE_CPU)
        return fb

    def mapframe_rgba8(self, flip_vertical=True, device=False):
        """the current frame as packed RGBA8, converted on the GPU exactly like the reference's image_to_rgba8
        (imageio.cpp:146-181; renderbatch saves its PNG from this, flipped).  Returns a (H, W, 4) uint8 numpy array (host) or
        torch tensor (device=True); valid until the next call."""
        ptr, nb = C.c_void_p(), C.c_size_t()
        L.check(self._lib.ovr_hip_mapframe_rgba8(self._h, L.MEM_DEVICE if device else L.MEM_HOST, 1 if flip_vertical else 0, C.byref(ptr), C.byref(nb)))
        w, h = self._fbsize
        if device:
            import torch
            return torch.as_tensor(_DevicePtr(ptr.value, (h, w, 4), typestr="|u1"), device=torch.device("cuda", self.device_id))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(h, w, 4))

    def mapframe_rgba16f(self, flip_vertical=True, device=False):
        """the current frame as RGBA half (IEEE binary16 bit patterns, (H, W, 4) uint16), converted on the GPU with the float ->
        half rule of the reference's EXR writer (imageio.cpp:15-83, tinyexr); valid until the next call."""
        ptr, nb = C.c_void_p(), C.c_size_t()
        L.check(self._lib.ovr_hip_mapframe_rgba16f(self._h, L.MEM_DEVICE if device else L.MEM_HOST, 1 if flip_vertical else 0, C.byref(ptr), C.byref(nb)))
        w, h = self._fbsize
        if device:
            import torch
            return torch.as_tensor(_DevicePtr(ptr.value, (h, w, 4), typestr="<i2"), device=torch.device("cuda", self.device_id))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint16)), shape=(h, w, 4))

    def save_image(self, path, flip_vertical=True):
        """ovr::save_image of the reference (imageio.cpp:264-284) for the current frame: the extension picks the format -
        "exr" (RGBA half, rows flipped before the write), "png" / "jpg" (image_to_rgba8, rows flipped on write).  The pixel
        conversion runs on the GPU (mapframe_rgba16f / mapframe_rgba8), imageio.py writes the file."""
        from . import imageio
        ext = path.rsplit(".", 1)[-1].lower()
        if ext == "exr":
            imageio.save_exr(path, np.array(self.mapframe_rgba16f(flip_vertical=flip_vertical), copy=True))
        elif ext in ("jpg", "jpeg"):
            imageio.save_jpg(path, np.array(self.mapframe_rgba8(flip_vertical=flip_vertical), copy=True))
        else:
            imageio.save_png(path, np.array(self.mapframe_rgba8(flip_vertical=flip_vertical), copy=True))

    # ---- getters ------------------------------------------------------------------------------------------------
    @property
    def render_time(self):
        """MainRenderer::render_time (renderer.h:87): accumulated milliseconds inside render()."""
        return float(self._lib.ovr_hip_render_time_ms(self._h))

    def unsafe_get_fbsize(self):
        return self._fbsize

    def unsafe_get_variance(self):
        return self.variance

    def stats(self):
        s = L.Stats()
        L.check(self._lib.ovr_hip_get_stats(self._h, C.byref(s)))
        return s

    def group_info(self):
        """(devices, gather: 0 none / 1 peer copies / 2 RCCL, host milliseconds of the last frame's gather tail)"""
        n, kind, ms = C.c_int32(), C.c_int32(), C.c_double()
        L.check(self._lib.ovr_hip_group_info(self._h, C.byref(n), C.byref(kind), C.byref(ms)))
        return n.value, kind.value, ms.value

    def group_host_times(self):
        """host microseconds of the last frame's steps on the leader's thread: (enqueue, ship, finish, scatter); zeros without a group (ABI v10)"""
        out = (C.c_double * 4)()
        L.check(self._lib.ovr_hip_group_host_times(self._h, out))
        return tuple(out)

    def upload_times(self):
        """milliseconds of the last ovr_hip_set_volume: dict(total, alloc, copy, kernels) (ABI v10)"""
        out = (C.c_double * 4)()
        L.check(self._lib.ovr_hip_get_upload_times(self._h, out))
        return dict(total_ms=out[0], alloc_ms=out[1], copy_ms=out[2], kernels_ms=out[3])

    def member_stats(self, member):
        s = L.Stats()
        L.check(self._lib.ovr_hip_get_member_stats(self._h, int(member), C.byref(s)))
        return s

    # ---- stand-alone pieces for known-answer tests ----------------------------------------------------------------
    def sparse_mask(self, frame_index):
        import torch
        w, h = self._fbsize
        out = torch.empty(w * h * 2, dtype=torch.int32, device=torch.device("cuda", self.device_id))
        n = C.c_int64()
        L.check(self._lib.ovr_hip_sparse_mask(self._h, int(frame_index), C.c_void_p(out.data_ptr()), out.numel() * 4, C.byref(n)))
        return out[: n.value].cpu().numpy()

    def tea_floats(self, v0v1):
        import torch
        dev = torch.device("cuda", self.device_id)
        st = torch.as_tensor(np.ascontiguousarray(v0v1, dtype=np.uint32).view(np.int32)).to(dev)
        out = torch.empty(st.numel(), dtype=torch.float32, device=dev)
        L.check(self._lib.ovr_hip_tea_floats(self._h, C.c_void_p(st.data_ptr()), C.c_void_p(out.data_ptr()), st.numel() // 2))
        return out.cpu().numpy(), st.cpu().numpy().view(np.uint32)


    def pow_floats(self, x, y, which=0):
        """the kernels' `__powf(x, y)` on the device (known-answer entry): which = 0 the pow this library was built with, 1 the deterministic pair"""
        import torch
        dev = torch.device("cuda", self.device_id)
        xd = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
        yd = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32)).to(dev)
        out = torch.empty(xd.numel(), dtype=torch.float32, device=dev)
        L.check(self._lib.ovr_hip_pow_floats(self._h, C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), C.c_void_p(out.data_ptr()), xd.numel(), int(which)))
        return out.cpu().numpy()


def create_renderer(name: str, device_id: int = 0, devices=None):
    """create_renderer(name) (reference ovr/renderer.cpp:42-61).  Only "hip" exists here; anything else raises the
    same way the reference's factory does for an unknown device.  devices = [ordinals]: an in-process device group."""
    if name == "hip":
        return DeviceHIP(device_id, devices)
    raise RuntimeError(f"OVR ERROR: Could not find device_{name} (only the 'hip' device is built)")
