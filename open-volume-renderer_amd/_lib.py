"""ctypes binding of the C ABI in include/ovr_hip.h (libovr_hip.so, built for gfx950 by csrc/Makefile).

There is no CPU fallback: if the library is missing, or no MI355X is present when a renderer is created, the
call fails loudly (RuntimeError), exactly like the reference's device throws std::runtime_error."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OVR_HIP_LIBRARY: development override (A/B runs of differently built kernels); the default is the in-tree build
LIB_PATH = os.environ.get("OVR_HIP_LIBRARY") or os.path.join(_HERE, "libovr_hip.so")

# numeric values of ovr::ValueType (ovr/scene.h:32-53)
TYPE_UINT8, TYPE_INT8 = 100, 101
TYPE_UINT16, TYPE_INT16 = 200, 201
TYPE_UINT32, TYPE_INT32 = 300, 301
TYPE_FLOAT, TYPE_DOUBLE = 400, 500
MEM_HOST, MEM_DEVICE = 0, 1
SHADE_NONE, SHADE_GRADIENT, SHADE_FULL = 0, 1, 2
GRID_CELL_CENTRED, GRID_VERTEX_CENTRED = 0, 1
PIPELINE_AUTO, PIPELINE_IN_PLACE, PIPELINE_POOLED = 0, 1, 2
JITTER_TEA, JITTER_BLUE_NOISE = 0, 1
CONVERGENCE_OFF, CONVERGENCE_ESTIMATE, CONVERGENCE_ADAPTIVE = 0, 1, 2
RECONSTRUCT_OFF, RECONSTRUCT_FILL = 0, 1
SHADOWS_MARCHED, SHADOWS_CACHED, SHADOWS_SUPPLIED = 0, 1, 2
PROJECT_OFF, PROJECT_MAXIMUM, PROJECT_MINIMUM, PROJECT_MEAN = 0, 1, 2, 3
LAYOUT_AUTO, LAYOUT_GENERAL, LAYOUT_THIN, LAYOUT_THIN_T, LAYOUT_QUAD = -1, 0, 1, 2, 3
# the ABI these ctypes structures describe: load() refuses a library of another version (ovr_hip_get_stats would write past them)
EXPECTED_ABI = 11


class Stats(C.Structure):
    _fields_ = [
        ("rays", C.c_uint64),
        ("samples", C.c_uint64),
        ("shaded_samples", C.c_uint64),
        ("shadow_samples", C.c_uint64),
        ("active_pixels", C.c_uint64),
        ("kernel_ms", C.c_double),
        ("render_ms", C.c_double),
        ("frame_index", C.c_int32),
        ("pipeline", C.c_int32),
        ("march_ms", C.c_double),
        ("shade_ms", C.c_double),
        ("composite_ms", C.c_double),
        ("pool_chunks", C.c_uint64),
        ("skipped_samples", C.c_uint64),
        ("skipped_shadow_samples", C.c_uint64),
        ("layout", C.c_int32),
        ("stale_tiles", C.c_int32),
        ("lds_fallback_taps", C.c_uint64),
        ("lds_unstaged_rounds", C.c_uint64),
        ("lds_rounds", C.c_uint64),
        ("skipping_kernels", C.c_int32),
        ("tuning", C.c_int32),
        ("replicas_building", C.c_int32),
    ]


class VolumeInfo(C.Structure):
    _fields_ = [
        ("dims", C.c_int32 * 3),
        ("value_type", C.c_int32),
        ("resident_bytes", C.c_uint64),
        ("data_lower", C.c_float),
        ("data_upper", C.c_float),
        ("tf_lower", C.c_float),
        ("tf_upper", C.c_float),
    ]


class Convergence(C.Structure):
    _fields_ = [
        ("error", C.c_float),
        ("threshold", C.c_float),
        ("mode", C.c_int32),
        ("valid", C.c_int32),
        ("frames", C.c_int32),
        ("blocks", C.c_int32),
        ("active_blocks", C.c_int32),
        ("retired_blocks", C.c_int32),
    ]


class Reconstruction(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("valid", C.c_int32),
        ("levels", C.c_int32),
        ("sampled_pixels", C.c_uint64),
        ("filled_pixels", C.c_uint64),
        ("reconstruct_ms", C.c_double),
    ]


class Lighting(C.Structure):
    _fields_ = [
        ("direction", C.c_float * 3),
        ("intensity", C.c_float),
        ("ambient", C.c_float),
        ("diffuse", C.c_float),
        ("specular", C.c_float),
        ("shininess", C.c_float),
        ("is_reference", C.c_int32),
    ]


class ClipBox(C.Structure):
    _fields_ = [
        ("enabled", C.c_int32),
        ("lower", C.c_float * 3),
        ("upper", C.c_float * 3),
        ("object_lower", C.c_float * 3),
        ("object_upper", C.c_float * 3),
    ]


class ShadowCache(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("cell", C.c_int32),
        ("dims", C.c_int32 * 3),
        ("valid", C.c_int32),
        ("builds", C.c_uint64),
        ("build_shadow_samples", C.c_uint64),
        ("bytes", C.c_uint64),
        ("build_ms", C.c_double),
    ]


class Projection(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("range_skipping", C.c_int32),
    ]


MAX_ISOVALUES = 4


class Isosurfaces(C.Structure):
    _fields_ = [
        ("n", C.c_int32),
        ("isovalues", C.c_float * MAX_ISOVALUES),
        ("range_skipping", C.c_int32),
    ]


class IsosurfaceLayers(C.Structure):
    _fields_ = [
        ("n", C.c_int32),
        ("isovalues", C.c_float * MAX_ISOVALUES),
        ("opacities", C.c_float * MAX_ISOVALUES),
        ("translucent", C.c_int32),
        ("range_skipping", C.c_int32),
    ]


MAX_SLICES = 4


class Slice(C.Structure):
    _fields_ = [
        ("point", C.c_float * 3),
        ("normal", C.c_float * 3),
        ("thickness", C.c_float),
        ("mode", C.c_int32),
    ]


class CommittedSlice(C.Structure):
    _fields_ = [
        ("normal", C.c_float * 3),
        ("c", C.c_float),
        ("thickness", C.c_float),
        ("mode", C.c_int32),
    ]


class Slices(C.Structure):
    _fields_ = [
        ("n", C.c_int32),
        ("slice", CommittedSlice * MAX_SLICES),
        ("walks", C.c_int32),
        ("range_skipping", C.c_int32),
    ]


SLICE_CONTEXT_OFF, SLICE_CONTEXT_FRONT = 0, 1


class SliceContext(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("opacity_scale", C.c_float),
        ("active", C.c_int32),
    ]


ISO_CONTEXT_OFF, ISO_CONTEXT_VOLUME = 0, 1


class IsosurfaceContext(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("opacity_scale", C.c_float),
        ("active", C.c_int32),
    ]


PREINTEGRATION_OFF, PREINTEGRATION_SEGMENTS = 0, 1


class Preintegration(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("active", C.c_int32),
        ("nodes", C.c_int32),
        ("subdivision", C.c_int32),
    ]


GRADIENT_OPACITY_OFF, GRADIENT_OPACITY_RAMP = 0, 1


class GradientOpacity(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("active", C.c_int32),
        ("lo", C.c_float),
        ("hi", C.c_float),
        ("inv_ramp", C.c_float),
    ]


MAX_DEPTH_OFF, MAX_DEPTH_ON = 0, 1


class MaxDepth(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("active", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
    ]


DEPTH_OUTPUT_OFF, DEPTH_OUTPUT_ON = 0, 1


class DepthOutput(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("active", C.c_int32),
        ("limited", C.c_int32),
        ("threshold", C.c_float),
    ]


MAX_AO_SAMPLES, AO_ROTATIONS = 16, 16


class AmbientOcclusion(C.Structure):
    _fields_ = [
        ("samples", C.c_int32),
        ("distance", C.c_float),
        ("rotations", C.c_int32),
        ("active", C.c_int32),
    ]


CAMERA_PERSPECTIVE, CAMERA_ORTHOGRAPHIC = 0, 1


class CameraState(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("eye", C.c_float * 3),   # `from` in the header (a Python keyword)
        ("at", C.c_float * 3),
        ("up", C.c_float * 3),
        ("fovy", C.c_float),
        ("height", C.c_float),
        ("pos", C.c_float * 3),
        ("dir", C.c_float * 3),
        ("hor", C.c_float * 3),
        ("ver", C.c_float * 3),
    ]


# every symbol include/ovr_hip.h declares: name -> (restype, argtypes)
_F3 = C.POINTER(C.c_float)
_H = C.c_void_p
SYMBOLS = {
    "ovr_hip_last_error": (C.c_char_p, []),
    "ovr_hip_abi_version": (C.c_int, []),
    "ovr_hip_create": (C.c_int, [C.POINTER(_H), C.c_int]),
    "ovr_hip_destroy": (None, [_H]),
    "ovr_hip_create_group": (C.c_int, [C.POINTER(_H), C.POINTER(C.c_int32), C.c_int32]),
    "ovr_hip_group_info": (C.c_int, [_H, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "ovr_hip_group_host_times": (C.c_int, [_H, C.POINTER(C.c_double)]),
    "ovr_hip_get_upload_times": (C.c_int, [_H, C.POINTER(C.c_double)]),
    "ovr_hip_pow_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "ovr_hip_built_for_exact_parity": (C.c_int, []),
    "ovr_hip_get_member_stats": (C.c_int, [_H, C.c_int32, C.POINTER(Stats)]),
    "ovr_hip_rccl_selftest": (C.c_int, [C.c_int]),
    "ovr_hip_set_stream": (C.c_int, [_H, C.c_void_p]),
    "ovr_hip_set_volume": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), _F3, _F3]),
    "ovr_hip_set_grid_convention": (C.c_int, [_H, C.c_int]),
    "ovr_hip_set_transfer_function": (C.c_int, [_H, _F3, C.c_int32, _F3, C.c_int32, C.c_float, C.c_float]),
    "ovr_hip_set_camera": (C.c_int, [_H, _F3, _F3, _F3, C.c_float]),
    "ovr_hip_set_camera_orthographic": (C.c_int, [_H, _F3, _F3, _F3, C.c_float]),
    "ovr_hip_get_camera": (C.c_int, [_H, C.POINTER(CameraState)]),
    "ovr_hip_camera_rays": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]),
    "ovr_hip_set_fbsize": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "ovr_hip_set_sample_per_pixel": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_set_volume_sampling_rate": (C.c_int, [_H, C.c_float]),
    "ovr_hip_set_frame_accumulation": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_set_sparse_sampling": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_set_focus": (C.c_int, [_H, C.c_float, C.c_float, C.c_float, C.c_float]),
    "ovr_hip_set_noise_tile": (C.c_int, [_H, _F3, C.c_int32]),
    "ovr_hip_set_shading": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_set_shading_pipeline": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_set_empty_space_skipping": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_get_macrocells": (C.c_int, [_H, C.POINTER(C.c_int32), _F3, _F3, C.c_size_t]),
    "ovr_hip_set_image_shard": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ovr_hip_commit": (C.c_int, [_H]),
    "ovr_hip_render": (C.c_int, [_H]),
    "ovr_hip_render_async": (C.c_int, [_H]),
    "ovr_hip_sync": (C.c_int, [_H]),
    "ovr_hip_mapframe": (C.c_int, [_H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "ovr_hip_swap": (C.c_int, [_H]),
    "ovr_hip_render_time_ms": (C.c_double, [_H]),
    "ovr_hip_get_stats": (C.c_int, [_H, C.POINTER(Stats)]),
    "ovr_hip_owned_tiles": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32)]),
    "ovr_hip_pack_tiles": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "ovr_hip_unpack_tiles": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "ovr_hip_mapframe_rgba8": (C.c_int, [_H, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "ovr_hip_unpack_all_tiles": (C.c_int, [_H, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]),
    "ovr_hip_sparse_mask": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64)]),
    "ovr_hip_tea_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64]),
    "ovr_hip_set_pixel_jitter": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_set_lds_staging": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_set_phase_timing": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_query_addressing_mode": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.c_int32, C.c_int32, C.c_int32]),
    "ovr_hip_set_volume_layouts": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_set_layout_choice": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_get_volume_info": (C.c_int, [_H, C.POINTER(VolumeInfo)]),
    "ovr_hip_mapframe_rgba16f": (C.c_int, [_H, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "ovr_hip_set_convergence": (C.c_int, [_H, C.c_int32, C.c_float]),
    "ovr_hip_get_convergence": (C.c_int, [_H, C.POINTER(Convergence)]),
    "ovr_hip_get_convergence_blocks": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), _F3, C.POINTER(C.c_int32), C.c_size_t]),
    "ovr_hip_get_accumulation": (C.c_int, [_H, C.c_int32, C.c_int32, _F3, C.c_size_t]),
    "ovr_hip_set_reconstruction": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_get_reconstruction": (C.c_int, [_H, C.POINTER(Reconstruction)]),
    "ovr_hip_get_reconstruction_weights": (C.c_int, [_H, _F3, C.c_size_t]),
    "ovr_hip_get_reconstruction_gradient": (C.c_int, [_H, _F3, C.c_size_t]),
    "ovr_hip_set_light": (C.c_int, [_H, _F3, C.c_float]),
    "ovr_hip_set_material": (C.c_int, [_H, C.c_float, C.c_float, C.c_float, C.c_float]),
    "ovr_hip_get_lighting": (C.c_int, [_H, C.POINTER(Lighting)]),
    "ovr_hip_shade_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "ovr_hip_set_clip_box": (C.c_int, [_H, _F3, _F3]),
    "ovr_hip_get_clip_box": (C.c_int, [_H, C.POINTER(ClipBox)]),
    "ovr_hip_clip_intervals": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "ovr_hip_set_shadow_cache": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "ovr_hip_set_shadow_cache_values": (C.c_int, [_H, C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "ovr_hip_get_shadow_cache": (C.c_int, [_H, C.POINTER(ShadowCache)]),
    "ovr_hip_get_shadow_cache_values": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), _F3, _F3, C.c_size_t]),
    "ovr_hip_shadow_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "ovr_hip_set_projection": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_get_projection": (C.c_int, [_H, C.POINTER(Projection)]),
    "ovr_hip_project_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "ovr_hip_set_slices": (C.c_int, [_H, C.POINTER(Slice), C.c_int32]),
    "ovr_hip_get_slices": (C.c_int, [_H, C.POINTER(Slices)]),
    "ovr_hip_slice_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "ovr_hip_set_slice_context": (C.c_int, [_H, C.c_int32, C.c_float]),
    "ovr_hip_get_slice_context": (C.c_int, [_H, C.POINTER(SliceContext)]),
    "ovr_hip_slice_context_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "ovr_hip_set_isosurface_context": (C.c_int, [_H, C.c_int32, C.c_float]),
    "ovr_hip_get_isosurface_context": (C.c_int, [_H, C.POINTER(IsosurfaceContext)]),
    "ovr_hip_isosurface_context_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "ovr_hip_set_preintegration": (C.c_int, [_H, C.c_int32]),
    "ovr_hip_get_preintegration": (C.c_int, [_H, C.POINTER(Preintegration)]),
    "ovr_hip_get_preintegration_tables": (C.c_int, [_H, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_int32)]),
    "ovr_hip_preintegrated_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "ovr_hip_set_gradient_opacity": (C.c_int, [_H, C.c_int32, C.c_float, C.c_float]),
    "ovr_hip_get_gradient_opacity": (C.c_int, [_H, C.POINTER(GradientOpacity)]),
    "ovr_hip_gradient_opacity_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "ovr_hip_set_max_depth": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int32, C.c_int32]),
    "ovr_hip_get_max_depth": (C.c_int, [_H, C.POINTER(MaxDepth)]),
    "ovr_hip_get_max_depth_values": (C.c_int, [_H, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ovr_hip_max_depth_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "ovr_hip_set_depth_output": (C.c_int, [_H, C.c_int32, C.c_float]),
    "ovr_hip_get_depth_output": (C.c_int, [_H, C.POINTER(DepthOutput)]),
    "ovr_hip_depth_output_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float]),
    "ovr_hip_set_isosurfaces": (C.c_int, [_H, C.POINTER(C.c_float), C.c_int32]),
    "ovr_hip_get_isosurfaces": (C.c_int, [_H, C.POINTER(Isosurfaces)]),
    "ovr_hip_isosurface_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "ovr_hip_set_isosurface_layers": (C.c_int, [_H, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32]),
    "ovr_hip_get_isosurface_layers": (C.c_int, [_H, C.POINTER(IsosurfaceLayers)]),
    "ovr_hip_isosurface_layers_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "ovr_hip_set_ambient_occlusion": (C.c_int, [_H, C.c_int32, C.c_float]),
    "ovr_hip_get_ambient_occlusion": (C.c_int, [_H, C.POINTER(AmbientOcclusion)]),
    "ovr_hip_get_ambient_occlusion_directions": (C.c_int, [_H, C.POINTER(C.c_float), C.c_size_t]),
    "ovr_hip_isosurface_ao_floats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "ovr_hip_reconstruct_image": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "ovr_hip_update_volume": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ovr_hip_get_update_times": (C.c_int, [_H, C.POINTER(C.c_double)]),
    "ovr_hip_get_volume_layout": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
}

_lib = None


def load():
    """dlopen libovr_hip.so and bind every declared symbol; raises RuntimeError if the library or a symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found - build it with `make -C open-volume-renderer_amd/csrc` "
            "(or __graft_entry__.build()); this backend has no CPU fallback")
    # torch ships its own copy of the HIP runtime: if libovr_hip.so brings up /opt/rocm's first, a later torch.cuda
    # initialisation in the same process finds "No HIP GPUs" (seen on the GPU box).  Loading torch's libraries first makes
    # both share one runtime; hosts without torch (the C++ plugin) have only one runtime anyway.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"libovr_hip.so does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    abi = lib.ovr_hip_abi_version()
    if abi != EXPECTED_ABI:
        raise RuntimeError(f"{LIB_PATH} implements ABI version {abi}, this Python package describes version {EXPECTED_ABI}: rebuild the "
                           "library (make -C open-volume-renderer_amd/csrc) or update the package")
    _lib = lib
    return lib


def check(code):
    if code != 0:
        msg = load().ovr_hip_last_error()
        raise RuntimeError((msg or b"").decode("utf-8", "replace") or f"ovr_hip error {code}")
