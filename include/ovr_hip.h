/* ovr_hip.h - C ABI of the MI355X (gfx950) ray-marching backend for OVR's renderer API.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  Every entry point
 * replaces one member of the reference's device interface; `file:line` citations are relative to the
 * reference tree (VIDILabs/open-volume-renderer).  The reference-side binding (a ~180-line
 * `DeviceHIP : ovr::MainRenderer` compiled against the reference's own headers and exported as
 * `ovr_create_renderer__hip`, the symbol ovr/renderer.cpp:55-58 looks up) lives in plugin/device_hip.cpp
 * and is described in INTEGRATION.md.
 *
 * Error model: every function returns 0 on success and a negative OVR_HIP_E* code on failure;
 * ovr_hip_last_error() returns the message.  The reference reports errors as std::runtime_error
 * (ovr/common/cuda/cuda_misc.h:44-100); the C++ binding rethrows with the same text.
 *
 * Threading: like the reference (SURVEY.md 8b "Threading") setters may be called from any thread,
 * commit/render/mapframe/swap from one render thread at a time.
 */
#ifndef OVR_HIP_H
#define OVR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OVR_HIP_ABI_VERSION 11

/* error codes */
#define OVR_HIP_OK 0
#define OVR_HIP_EINVAL (-1)   /* bad argument (the reference throws std::runtime_error) */
#define OVR_HIP_EDEVICE (-2)  /* HIP runtime error / no gfx950 device */
#define OVR_HIP_ESTATE (-3)   /* call order violated (e.g. render before a volume was set) */

/* Scalar types: numeric values of ovr::ValueType, ovr/scene.h:32-53 */
#define OVR_HIP_TYPE_UINT8 100
#define OVR_HIP_TYPE_INT8 101
#define OVR_HIP_TYPE_UINT16 200
#define OVR_HIP_TYPE_INT16 201
#define OVR_HIP_TYPE_UINT32 300
#define OVR_HIP_TYPE_INT32 301
#define OVR_HIP_TYPE_FLOAT 400
#define OVR_HIP_TYPE_DOUBLE 500

/* where a buffer lives (mirrors CrossDeviceBuffer::Device, ovr/common/cross_device_buffer.h:22-27) */
#define OVR_HIP_MEM_HOST 0
#define OVR_HIP_MEM_DEVICE 1

/* shading modes.  FULL = what the reference's live marcher always does (shaders_raymarching.cu:124-158) */
#define OVR_HIP_SHADE_NONE 0     /* absorption + emission: value tap + TF only (BASELINE config 2)        */
#define OVR_HIP_SHADE_GRADIENT 1 /* + forward-difference gradient and |N.L| term, no shadow march (config 3) */
#define OVR_HIP_SHADE_FULL 2     /* + per-sample shadow march toward the fixed directional light            */

/* grid convention */
#define OVR_HIP_GRID_CELL_CENTRED 0   /* in-tree OptiX device (default)        */
#define OVR_HIP_GRID_VERTEX_CENTRED 1 /* OSPRay wrapper's structuredRegular     */

typedef struct ovr_hip_renderer ovr_hip_renderer; /* opaque; one per GPU */

/* counters of the most recent render() (the metric's "sample" = one primary marching-loop iteration) */
typedef struct ovr_hip_stats {
  uint64_t rays;            /* primary rays (pixels x spp) launched by this rank                             */
  uint64_t samples;         /* primary marching-loop iterations                                               */
  uint64_t shaded_samples;  /* primary samples with corrected opacity > 0 (gradient/shadow taps executed)    */
  uint64_t shadow_samples;  /* shadow-march iterations executed                                               */
  uint64_t active_pixels;   /* pixels rendered (sparse sampling / tile sharding reduce it below W*H)         */
  double kernel_ms;         /* hipEvent time of the ray-march kernel of the last render()                     */
  double render_ms;         /* wall time of the last render() call, as DeviceOptix7::render measures it       */
  int32_t frame_index;      /* accumulation frame counter after the last render (device_impl.cpp:241)         */
  int32_t pipeline;         /* 1 = shaded in place, 2 = pooled (march -> shade -> composite kernels)          */
  double march_ms;          /* hipEvent time of the primary-march kernel (== kernel_ms when shading in place)  */
  double shade_ms;          /* pooled pipeline: the persistent shading kernel                                  */
  double composite_ms;      /* pooled pipeline: composite + counter reduction                                  */
  uint64_t pool_chunks;     /* pooled pipeline: 2 KiB request chunks used by the frame                         */
  uint64_t skipped_samples; /* empty-space skipping: primary iterations whose voxel fetch was skipped (not in `samples`) */
  uint64_t skipped_shadow_samples; /* same for shadow-march iterations (not in `shadow_samples`)                 */
  int32_t layout;           /* which resident layout of the volume the frame read: 0 general, 1 thin, 2 thin transposed, 3 quad */
  int32_t stale_tiles;      /* 1: this frame was rendered again (request-pool overflow) AFTER ovr_hip_pack_tiles had packed it - discard that payload */
  uint64_t lds_fallback_taps;   /* LDS-staged bricks: taps of live samples that fell outside the staged box (read from L1/L2 instead) */
  uint64_t lds_unstaged_rounds; /* LDS-staged bricks: workgroup rounds whose box exceeded the LDS budget (ordinary path)            */
  uint64_t lds_rounds;          /* LDS-staged bricks: workgroup rounds in total                                                      */
  int32_t skipping_kernels;     /* 1: the frame ran the empty-space-skipping kernels; 0: the plain ones - skipping disabled, or enabled but
                                   suspended because the last probed frame skipped < 10 % of its sample steps (probed again after 32 ... 256
                                   frames and on every transfer-function / volume change; the frames are bit-identical either way)      */
  int32_t tuning;               /* automatic layout / pipeline (ABI v7): 0 = the frame ran what the rules say (camera direction, share of
                                   shaded samples), 1 = it was a probe (a shade-heavy configuration: the other pipeline and the general / quad
                                   layouts are timed, two frames each), 2 = it ran the measured winner (kept until the configuration changes) */
  int32_t replicas_building;    /* ABI v8: replicas of the volume still being built in the background when the frame finished (the frame
                                   read the general layout meanwhile - the same frame bit for bit; see ovr_hip_set_volume_layouts) */
} ovr_hip_stats;

const char* ovr_hip_last_error(void);
int ovr_hip_abi_version(void);

/* replaces create_renderer("hip") / new DeviceOptix7 + Impl::init (ovr/renderer.cpp:42-61, device_impl.cpp:70-100).
 * device_id = HIP device ordinal; the reference hard-codes 0 (device_impl.cpp:371-372). */
int ovr_hip_create(ovr_hip_renderer** out, int device_id);
void ovr_hip_destroy(ovr_hip_renderer* r);

/* ABI v8 - several GPUs behind ONE handle, in one process (north_star: "apps run unmodified ... the 8 GPUs of one node shard
 * the image plane into tiles with a final RCCL gather over xGMI").  The reference's device knows one GPU (device_impl.cpp:371-372) and its
 * apps create one renderer (apps/main_batch.cpp:240-318, apps/main_app.cpp:233-278): the returned handle is used exactly like the one of
 * ovr_hip_create - every setter, commit, render, mapframe, swap - and drives n_devices renderers, one per listed device: the volume is
 * replicated, device k renders the image tiles (tx + ty) % n == k (16 x 16 pixels; OVR_HIP_TILE=WxH, or ovr_hip_set_image_shard(r, 0, 1,
 * w, h)), and at the end of every frame the tiles of devices 1 ... n-1 travel to device_ids[0] - ncclSend / ncclRecv between the
 * communicators of this process (librccl is loaded at run time) when the devices are distinct, peer-to-peer copies otherwise or when RCCL is
 * absent (OVR_HIP_GATHER=rccl|copy forces one) - where one launch per layer scatters them into the leader's framebuffer.  Pixels, TEA seeds and
 * accumulation are per pixel: the frame is the single-device frame bit for bit.  A device may be listed more than once (a rehearsal on one
 * card).  n_devices == 1 is ovr_hip_create.  ovr_hip_get_stats sums the members' counters and reports the slowest member's times;
 * OVR_HIP_MAP_GRAD=0 leaves the gradient layer out of the gather (it is then valid for device 0's tiles only). */
int ovr_hip_create_group(ovr_hip_renderer** out, const int32_t* device_ids, int32_t n_devices);
/* n_devices (1 for an ordinary renderer), how the tiles travel (0 = no group, 1 = peer copies, 2 = RCCL), and the host time the last frame
 * spent after its slowest member had finished (waiting for the shipments + the scatter), milliseconds; any pointer may be NULL */
int ovr_hip_group_info(const ovr_hip_renderer* r, int32_t* n_devices, int32_t* gather_kind, double* gather_ms);
/* diagnostic: the RCCL entry points a device group uses (ncclCommInitAll, ncclGroupStart / End, ncclSend, ncclRecv on a stream), exercised on
 * ONE device - a communicator of one rank sends 256 KiB to itself.  0 = they work; OVR_HIP_ESTATE = librccl.so is not loadable (groups use peer copies) */
int ovr_hip_rccl_selftest(int device_id);
/* ABI v10: host time of the last frame's steps on the calling (leader's) thread, microseconds: [0] launching every member's frame (each follower on
 * its own host thread, the leader on this one), [1] packing + shipping the followers' tiles, [2] every member's frame to its end, [3] waiting for the
 * shipments + the scatter on the leader.  Zeros for an ordinary renderer.  Round 4 drove all members from one thread: [0] was 225 us at 8 members. */
int ovr_hip_group_host_times(const ovr_hip_renderer* r, double out_us[4]);
/* the counters of ONE member's last frame (member 0 = the leader's own tiles) */
int ovr_hip_get_member_stats(const ovr_hip_renderer* r, int32_t member, ovr_hip_stats* out);

/* Use a caller-owned hipStream_t for all device work (e.g. torch's current stream); NULL = private streams,
 * one per framebuffer set like DoubleBufferObject (optix7_common.h:328-414). */
int ovr_hip_set_stream(ovr_hip_renderer* r, void* hip_stream);

/* replaces Impl::buildScene + StructuredRegularVolume::load_from_array3d_scalar + CreateArray3DScalarOptix7
 * (device_impl.cpp:283-302, volume.cpp:181-257, array.cpp:287-351).  `data` = dims[0]*dims[1]*dims[2] scalars,
 * x fastest.  The volume is re-laid out into HBM-resident bricks; `data` is not referenced after the call returns. */
int ovr_hip_set_volume(ovr_hip_renderer* r, const void* data, int mem_kind, int value_type, const int32_t dims[3],
                       const float grid_origin[3], const float grid_spacing[3]);
/* ABI v10: where the last ovr_hip_set_volume spent its time, milliseconds: [0] the whole call (a device group: over all members, which upload side by
 * side), [1] allocation (a FRESH hipMalloc costs 30-60 ms per GiB on this platform - the driver maps and clears the pages; C4's 21.5 GB layout: 0.5-1.2 s
 * in a new process, 0.1 ms when the runtime still holds a freed block of that size), [2] copies into the device (host input: through a 1 GiB staging buffer;
 * a device array on another GPU: peer copies), [3] kernels (re-bricking, macrocell ranges, data range; layouts mode 2: the replicas) */
int ovr_hip_get_upload_times(const ovr_hip_renderer* r, double out_ms[4]);
/* extension (within ABI v11): replaces the voxels [lower, lower + extent) of the RESIDENT volume - a step of a time series, a
 * simulation's new state, an edit - in place.  `data` = extent[0]*extent[1]*extent[2] scalars, x fastest, of the value_type the volume was set with; it
 * is not referenced after the call returns.  Immediate like ovr_hip_set_volume (a frame in flight is resolved first), but nothing is freed or
 * allocated - no layout, axis table or macrocell grid - and the device is not drained: box-restricted kernels rewrite the stored copies of the box's
 * voxels in the general layout and in every replica that is resident or being built, and recompute the macrocells whose window meets the box and the
 * data range.  Host input (or a device array on another GPU) travels through a staging buffer the renderer keeps and only ever grows.
 * DEFINITION: afterwards every observable - frames, gradient layer, counters, macrocell grids, ovr_hip_get_volume_info, the bytes of every resident
 * layout - is bit for bit what it would be after ovr_hip_set_volume with the patched array followed by the same setters and ovr_hip_commit.
 * Reset: the accumulation (with it the convergence estimate, its retired blocks and the reconstruction's counts), the tuner's measurement, the
 * adaptive-skipping probe, the pool's "roomy" mark.  Kept: the schedule, the queued and committed setters, the layouts' residency.
 * OVR_HIP_EINVAL (the volume intact and renderable): a null argument, a bad mem_kind, a value_type other than the resident one, an extent < 1, a box
 * that leaves the grid.  OVR_HIP_ESTATE: no volume is set.  A device group validates once, then updates every member; a device failure on any member
 * after writing began leaves no member renderable (ovr_hip_set_volume's rule). */
int ovr_hip_update_volume(ovr_hip_renderer* r, const void* data, int mem_kind, int value_type, const int32_t lower[3], const int32_t extent[3]);
/* where the last ovr_hip_update_volume spent its time, milliseconds, like ovr_hip_get_upload_times: [0] the whole call, [1] allocation (0 unless the
 * staging buffer grew), [2] copies into the device, [3] kernels */
int ovr_hip_get_update_times(const ovr_hip_renderer* r, double out_ms[4]);
/* for known-answer tests, like ovr_hip_get_macrocells: the raw bytes of a resident layout (0 general ... 3 quad) of member `member` (0 for an ordinary
 * renderer), without the 64 bytes of slack behind it.  host == NULL only reports the size in *bytes.  OVR_HIP_ESTATE if that layout is not resident
 * (a planned replica is not built for this call); a replica under construction is waited for. */
int ovr_hip_get_volume_layout(ovr_hip_renderer* r, int32_t member, int32_t layout, void* host, size_t capacity_bytes, uint64_t* bytes);
int ovr_hip_set_grid_convention(ovr_hip_renderer* r, int convention);
/* diagnostic, pure host arithmetic (no device needed): the addressing mode the kernels would take for a volume of these dimensions and
 * type in the given layout (0 general ... 3 quad) with a transfer function of n_colors / n_alphas entries: 0 = 32-bit byte offsets,
 * 1 = 32-bit element offsets, 2 = 64-bit z table in LDS, 3 = computed 64-bit offsets (per-axis tables would not fit in the 160 KiB of LDS
 * next to the transfer function and the request queues: a dimension of tens of thousands of voxels).  < 0: no such layout for the type. */
int ovr_hip_query_addressing_mode(const int32_t dims[3], int value_type, int32_t layout, int32_t n_colors, int32_t n_alphas);
/* extension (MI355X: 288 GB of HBM traded for bandwidth): which layouts of the volume ovr_hip_set_volume keeps resident.
 * Besides the general layout (128-byte 3-D bricks) two "thin" replicas serve views whose rays run along a volume axis - 12 of
 * the reference's 21 shipped scene cameras - where rays are sparser than voxels and a general brick is mostly wasted (C3 front
 * view: 2.18 -> 1.69 ms per frame).  Frames are bit-identical whatever layout is read.  mode 0 = general only, 1 (default) =
 * thin replicas for float / uint16 volumes when all replicas fit in 40 % of the free HBM (x 3 - 4 of the volume's size),
 * 2 = always.  Takes effect at the next ovr_hip_set_volume.
 * Round 3: float volumes get a fourth layout under the same rule, the "quad" replica - every cell stores its 2 x 2 (x, y) voxels as 16
 * contiguous bytes (4 x the volume's size), so a trilinear tap is two 16-byte loads instead of four 8-byte ones.  Frames that shade every
 * sample (most shipped scenes; every frame at the scene files' sampling rate 4) are bound by the gather-instruction rate: -7 ... -16 % there. */
int ovr_hip_set_volume_layouts(ovr_hip_renderer* r, int32_t mode);
/* which resident layout a frame reads: -1 (default) = automatic - from the camera direction (a thin replica within ~21 degrees of an
 * axis, cos >= 0.93) and, for configurations whose shading taps outnumber their primary taps, MEASURED: the frames after the first try the
 * other pipeline and the general / quad layouts, two frames each, and the fastest is kept until the configuration changes
 * (ovr_hip_stats.tuning; OVR_HIP_TUNE=0 disables the measuring).  0 / 1 / 2 / 3 = forced: general, thin, thin transposed, quad (general
 * if that replica is not resident).  Applied at commit; does not reset the accumulation - every layout gives the same frame bit for bit. */
int ovr_hip_set_layout_choice(ovr_hip_renderer* r, int32_t choice);

/* replaces MainRenderer::set_transfer_function -> StructuredRegularVolume::set_transfer_function
 * (ovr/renderer.h:154-161, volume.cpp:110-129): colors = n_colors flat RGB triples, alphas = n_alphas flat
 * (position, alpha) pairs (position ignored, as in the reference), range in raw data units. */
int ovr_hip_set_transfer_function(ovr_hip_renderer* r, const float* colors_rgb, int32_t n_colors,
                                  const float* alphas_pos_alpha, int32_t n_alphas, float range_lo, float range_hi);

/* replaces MainRenderer::set_camera (ovr/renderer.h:140-152); fovy in degrees (scene.h:219 default 60) */
int ovr_hip_set_camera(ovr_hip_renderer* r, const float from[3], const float at[3], const float up[3], float fovy);
/* The orthographic camera (ovr::scene::Camera::type == ORTHOGRAPHIC, ovr/scene.h:207-230; open-volume-renderer_amd/camera.py is the normative arithmetic,
 * DESIGN.md section 18): parallel rays along normalize(at - from), one per pixel sample, starting on the image plane through `from`; `height` is the world
 * height of the image, height * width / height its width.  A queued value like the perspective camera's, in the same slot: ovr_hip_set_camera stays the
 * perspective setter and switches back.  Every kind of frame honours it (the march, the projections, the isosurfaces); a ray that the reference's box test
 * would let through an ignored slab from outside it (a direction component below FLT_MIN: EVERY ray of an axis view has two) is a miss under this camera.
 * The distances of the projection and isosurface layers are then planar depth.  EINVAL, the state kept: a null pointer, a height that is not finite or not > 0. */
#define OVR_HIP_CAMERA_PERSPECTIVE 0
#define OVR_HIP_CAMERA_ORTHOGRAPHIC 1
int ovr_hip_set_camera_orthographic(ovr_hip_renderer* r, const float from[3], const float at[3], const float up[3], float height);
/* the COMMITTED camera: what the setter was given (fovy of a perspective, height of an orthographic camera; the other is 0) and pos ... ver, the basis the
 * kernels read (zeros until a framebuffer size is committed) */
typedef struct ovr_hip_camera {
  int32_t kind;
  float from[3], at[3], up[3], fovy, height;
  float pos[3], dir[3], hor[3], ver[3];
} ovr_hip_camera;
int ovr_hip_get_camera(const ovr_hip_renderer* r, ovr_hip_camera* out);
/* ovr/renderer.h:135-138 */
int ovr_hip_set_fbsize(ovr_hip_renderer* r, int32_t width, int32_t height);
/* ovr/renderer.h:170-173 */
int ovr_hip_set_sample_per_pixel(ovr_hip_renderer* r, int32_t spp);
/* ovr/renderer.h:200-203 -> StructuredRegularVolume::set_sampling_rate (volume.cpp:156-162) */
int ovr_hip_set_volume_sampling_rate(ovr_hip_renderer* r, float rate);
/* ovr/renderer.h:195-198 */
int ovr_hip_set_frame_accumulation(ovr_hip_renderer* r, int32_t enabled);
/* ovr/renderer.h:180-183 */
int ovr_hip_set_sparse_sampling(ovr_hip_renderer* r, int32_t enabled);
/* ovr/renderer.h:163-168 */
int ovr_hip_set_focus(ovr_hip_renderer* r, float center_x, float center_y, float scale, float base_noise);
/* blue-noise / STBN tile used by the sparse-sampling mask: xy*xy*64 floats, layout [y][x][t]
 * (ovr/common/random/blue_noise.h:44-47,95-99).  The reference embeds the tile at build time (ovr/CMakeLists.txt:67-72). */
int ovr_hip_set_noise_tile(ovr_hip_renderer* r, const float* tile, int32_t xy);
/* extension: select the sub-mode BASELINE.json's configs name; default OVR_HIP_SHADE_FULL (= reference) */
int ovr_hip_set_shading(ovr_hip_renderer* r, int32_t mode);
/* extension: how shaded samples are processed.  0 = automatic (pooled, or in place once a frame shaded >= 50 % of its samples - back to
 * pooled below 35 %: ovr_hip_stats::pipeline says which ran), 1 = in place
 * (the tile's own wave shades its request batches), 2 = pooled (request chunks go through a global pool and are shaded
 * by a separate, load-balanced kernel).  Both produce bit-identical frames. */
int ovr_hip_set_shading_pipeline(ovr_hip_renderer* r, int32_t mode);
/* extension: empty-space skipping with the reference's macrocell grids (16^3 value-range cells +
 * per-TF max-opacity cells, ovr/devices/optix7/accel/sp_singlemc.cu:10-97 - the reference computes them but only its path
 * tracer uses them).  Samples whose cell has majorant 0 have opacity exactly 0: their voxel fetch is skipped, frames stay
 * bit-identical.  Off by default (the reference's ray marcher visits every sample).  While it is enabled the renderer keeps the
 * skipping kernels only where they pay: a frame that skipped < 10 % of its sample steps (a dense transfer function, a camera inside the
 * data - there the skipping kernels cost 20-50 % more than the plain ones) switches to the plain kernels and the skipping ones are
 * probed again later (ovr_hip_stats::skipping_kernels says which ran; OVR_HIP_SKIP_ADAPTIVE=0 keeps them on regardless). */
int ovr_hip_set_empty_space_skipping(ovr_hip_renderer* r, int32_t enabled);
/* extension (BASELINE C5, north_star "blue-noise jitter staged in LDS"): how the sub-pixel position of a sample is drawn.
 * 0 (default) = the reference: RandomTEA(frame_index, pixel_index), applied iff sample_per_pixel > 1
 * (shaders_raymarching.cu:336,351-357).  1 = blue-noise tile (ovr_hip_set_noise_tile; lookup as blue_noise.h:95-99): sample k
 * of frame f uses slice ((f - 1) * spp + k) % 64, xi_x = tile[y % xy][x % xy][slice], xi_y = the slice shifted by half a tile
 * in x and y; applied to EVERY sample, so 64 accumulated 1-spp frames give the 64-spp progressive image. */
#define OVR_HIP_JITTER_TEA 0
#define OVR_HIP_JITTER_BLUE_NOISE 1
int ovr_hip_set_pixel_jitter(ovr_hip_renderer* r, int32_t mode);
/* extension (north_star "volume brick-tiled into LDS"): the unshaded (OVR_HIP_SHADE_NONE), non-skipping march of a float volume
 * stages, once per round of 16 steps, every brick its 8x8-pixel workgroup can touch into LDS with whole-line loads and taps read
 * LDS.  Bit-identical frames.  0 = off (default: 2.3 - 3 x slower than the L1 path on its best case, profiles/r02_notes.md), 1 = on. */
int ovr_hip_set_lds_staging(ovr_hip_renderer* r, int32_t mode);
/* extension (ABI v9): per-phase device times.  1 (default): two more events are recorded between the frame's kernels and
 * ovr_hip_stats::march_ms / shade_ms / composite_ms say what each phase took; 0: those three read 0 and a frame is ~16 us shorter (hipEventRecord
 * costs on both sides of the queue: 8 % of a 0.2 ms frame, 4 % of one GPU's share of an 8-GPU frame).  kernel_ms (first to last event) is measured
 * either way.  Takes effect with the next frame launched; frames are identical.  The plugin switches it off (OVR_HIP_PHASE_TIMING=1 keeps it). */
int ovr_hip_set_phase_timing(ovr_hip_renderer* r, int32_t on);
/* downloads the macrocell grids (for known-answer tests): dims = cells per axis; minmax = 2 floats per cell, majorant = 1 */
int ovr_hip_get_macrocells(ovr_hip_renderer* r, int32_t dims[3], float* minmax_host, float* majorant_host, size_t capacity_cells);
/* extension (multi-GPU): this renderer draws only the image tiles owned by `rank` of `world`;
 * owner(tile_x, tile_y) = (tile_x + tile_y) % world.  world = 1 restores the single-GPU behaviour. */
int ovr_hip_set_image_shard(ovr_hip_renderer* r, int32_t rank, int32_t world, int32_t tile_w, int32_t tile_h);

/* ABI v11 - convergence estimate and adaptive refinement.  The renderer interface has a convergence number -
 * MainRenderer::unsafe_get_variance(), ovr/renderer.h:124-127: the title bar of the interactive app, the stop criterion of the batch app's
 * progressive loop, apps/main_batch.cpp:211-215 - that the reference's OptiX device leaves at 0 (device_impl.cpp:266).  Defined while frames
 * accumulate and sparse sampling is off, from the second accumulated frame on.  Beside the accumulation buffer A the renderer keeps H, the sum of the
 * even-numbered frames; after an even frame n, per pixel (IEEE float, in this order)
 *     m = A / n, h = H / (n / 2) per channel;  d = ((|m_r - h_r| + |m_g - h_g|) + |m_b - h_b|) + |m_a - h_a|;  s = ((m_r + m_g) + m_b) + m_a;
 *     e = s > 0 ? d / sqrtf(s) : 0
 * and per 8x8-pixel block E_b = T(e) / P: T the balanced pairwise tree over the 64 pixels in the order 8 * (y & 7) + (x & 7), P the pixels of the block
 * that lie inside the image and belong to this renderer (pixels that do not contribute 0).  The frame error is the largest E_b.  It has the shape of
 * OSPRay's tile error (the whole accumulation against half of it, normalised by the root of the brightness) and is NOT claimed to equal its value.
 * open-volume-renderer_amd/convergence.py is the same arithmetic in numpy.
 *   OFF       today's behaviour: no buffer, no launch
 *   ESTIMATE  every frame is bit-identical to OFF; one more read-modify-write of 32 B per pixel and the estimate's kernels on even frames
 *   ADAPTIVE  + after an even frame n every active block with E_b <= threshold is RETIRED: it is no longer marched, keeps n_b = n, and in every later frame
 *             its pixels are written as A / n_b - and its gradient pixels as frame n_b left them - into the framebuffer set that frame renders into; it
 *             stays retired until the accumulation is reset.  ovr_hip_stats then counts what was marched.  When every block is retired a frame is that
 *             one small kernel.  A retired block keeps its E_b: frame error <= threshold exactly when every block is retired.
 * Queued like every setter, applied at commit; every call resets the accumulation.  EINVAL: unknown mode, a negative or non-finite threshold.
 * ovr_hip_render_async in these modes, as always, resolves the previous frame (reads its estimate and active count) before it launches the next. */
#define OVR_HIP_CONVERGENCE_OFF 0
#define OVR_HIP_CONVERGENCE_ESTIMATE 1
#define OVR_HIP_CONVERGENCE_ADAPTIVE 2
int ovr_hip_set_convergence(ovr_hip_renderer* r, int32_t mode, float threshold);

typedef struct ovr_hip_convergence {
  float error;            /* frame error; +inf while valid == 0 */
  float threshold;
  int32_t mode, valid;    /* valid: 0 before the second accumulated frame, without accumulation, with sparse sampling, with the mode OFF */
  int32_t frames;         /* the even frame the estimate belongs to (on an odd frame: the one before it) */
  int32_t blocks, active_blocks, retired_blocks; /* owned 8x8 blocks that a ray can meet (the others are never marched and have E_b = 0); a device
                                                     group: summed over its members, error = the largest member's */
} ovr_hip_convergence;
int ovr_hip_get_convergence(const ovr_hip_renderer* r, ovr_hip_convergence* out);
/* for known-answer tests, like ovr_hip_get_macrocells.  dims = blocks per axis (ceil(W / 8), ceil(H / 8)); error_host[bx + by * dims[0]] = E_b,
 * frames_host = n_b, negated when the block is retired; blocks this renderer does not own or that no ray meets read error 0, frames 0.
 * member: as ovr_hip_get_member_stats (0 for an ordinary renderer).  Either output may be NULL. */
int ovr_hip_get_convergence_blocks(ovr_hip_renderer* r, int32_t member, int32_t dims[2], float* error_host, int32_t* frames_host, size_t capacity_blocks);
/* the accumulation buffers, W*H*4 floats: which = 0: A, 1: H (ESTATE while the mode is OFF) */
int ovr_hip_get_accumulation(ovr_hip_renderer* r, int32_t member, int32_t which, float* host, size_t capacity_floats);

/* Pull-push reconstruction (added within ABI v11: new entry points and a new struct only, nothing that existed changed its layout or meaning;
 * a library without them fails to load in _lib.py by the missing symbols) - pull-push reconstruction of sparse-sampled frames.  A frame rendered with sparse sampling on is mostly holes: the pixels
 * the mask drops are exactly 0, and with accumulation a pixel sampled in k of n frames shows A / n, dimmed by k / n.  With the mode FILL such a frame is
 * completed on the device before anything maps it.  N(p) counts the frames that sampled pixel p (this frame alone without accumulation, since the last
 * reset with it); with accumulation G accumulates the gradient layer of the sampled pixels as A accumulates RGBA.  Level 0 of a pyramid is
 *     v0(p) = the framebuffer's pixel (without accumulation) or N > 0 ? (A / N, G / N) : 0;   w0(p) = N > 0 and all seven channels finite ? 1 : 0
 * a PULL halves the resolution up to 1 x 1 - a texel is the mean of its valid children (pairwise sums, x first; invalid children contribute a selected
 * +0) and is valid when one of them is - and a PUSH comes back down: a texel without data takes the bilinear interpolation (weights 0.75 / 0.25) of the
 * completed coarser level, a texel with data keeps its value.  On level 0 every pixel with N > 0 keeps v0 bit for bit (a non-finite sample stays where it
 * is and spreads nowhere), every other pixel is filled; RGBA and the gradient layer of the set the frame rendered into are written, so mapframe,
 * mapframe_rgba8 / rgba16f and save_image see the filled frame.  open-volume-renderer_amd/reconstruction.py is this arithmetic in numpy, the normative
 * text: the kernels agree with it bit for bit.
 *   OFF   today's behaviour: no buffer, no launch
 *   FILL  acts on frames rendered with sparse sampling on; a dense frame is bit-identical to OFF, with the same counters and launches
 * Queued like every setter, applied at commit; every call resets the accumulation.  EINVAL: unknown mode.  ESTATE: FILL on a device group of more than one
 * device (use ovr_hip_reconstruct_image on the assembled frame).  A renderer with an image shard (world > 1) leaves its frames alone (valid = 0). */
#define OVR_HIP_RECONSTRUCT_OFF 0
#define OVR_HIP_RECONSTRUCT_FILL 1
int ovr_hip_set_reconstruction(ovr_hip_renderer* r, int32_t mode);

typedef struct ovr_hip_reconstruction {
  int32_t mode, valid;      /* valid: 1 when the last frame was reconstructed; 0: mode OFF, sparse sampling off, an image shard */
  int32_t levels;           /* of the pyramid, the image (level 0) included; 0 while valid == 0 */
  uint64_t sampled_pixels;  /* pixels with N > 0 */
  uint64_t filled_pixels;   /* the others: W * H - sampled_pixels */
  double reconstruct_ms;    /* device time of the reconstruction's kernels; measured only while phase timing is on (else 0); never part of kernel_ms */
} ovr_hip_reconstruction;
int ovr_hip_get_reconstruction(const ovr_hip_renderer* r, ovr_hip_reconstruction* out);
/* for known-answer tests: N (W*H floats) and G (W*H*3 floats; ESTATE unless the last reconstructed frame accumulated).  ESTATE while the mode is OFF. */
int ovr_hip_get_reconstruction_weights(ovr_hip_renderer* r, float* host, size_t capacity_floats);
int ovr_hip_get_reconstruction_gradient(ovr_hip_renderer* r, float* host, size_t capacity_floats);
/* the same kernels on a caller's device image, in place: rgba_device W*H*4 floats, grad_device W*H*3 floats or NULL, weight_device W*H floats
 * (> 0 = sampled; not modified).  Stand-alone: needs no volume and no committed framebuffer; returns when the image is complete.  What the gathering
 * rank of a multi-process run calls on the assembled frame. */
int ovr_hip_reconstruct_image(ovr_hip_renderer* r, float* rgba_device, float* grad_device, const float* weight_device, int32_t width, int32_t height);

/* Light and material (added within ABI v11 like the reconstruction above: new entry points and a new struct only, nothing that existed
 * changed its layout or meaning; a library without them fails to load in _lib.py by the missing symbols).  The renderer interface has seven lighting controls - MainRenderer::set_light_phi / _theta /
 * _intensity, set_mat_ambient / _diffuse / _specular / _shininess, ovr/renderer.h:210-248, the sliders of the interactive app - that the reference's OptiX
 * device never reads: its light is a literal (params.h:79) and so is its shade expression (shaders_raymarching.cu:138,156-157).  Here they are real, and
 * until one of the two setters is called every frame, counter and time is what the literals give.
 *   direction  a world-space vector TOWARDS the light, any length; normalised on the host as the literal is.  NULL = the reference's literal.
 *              The interface's angles, in degrees, mean (sin phi cos theta, sin phi sin theta, cos phi): the app's defaults (99.53, 112.2) lie 0.15
 *              degrees from the literal.  The shadow march and the shade order by light beams follow the direction.
 *   intensity  the reference's light_rgb = 2 is intensity 1
 *   shade      per shaded sample, IEEE float in this order (n the world normal, L the unit light, I2 = 2 * intensity, shadow = 0 under SHADE_GRADIENT):
 *                  cosNL = |L . n|;  d = (diffuse * cosNL) * I2
 *                  if specular > 0:  V = normalize(camera - position), H = normalize(L + V), cosNH = |H . n|,
 *                                    sp = cosNH >= 2^-126 ? exp2(shininess * log2(cosNH)) : 0,  d = d + (specular * sp) * I2
 *                  shade = ambient + d * (1 - shadow)
 *              (0.5, 0.5, 0, any shininess) at intensity 1 is the reference's expression operation for operation.  open-volume-renderer_amd/lighting.py
 *              is this arithmetic in numpy, the normative text; the exact-parity build agrees with it bit for bit.
 * Queued like every setter, applied at commit; a CHANGED value resets the accumulation and voids what the layout / pipeline tuner measured.  EINVAL: a
 * zero, non-finite or not normalisable direction; a negative or non-finite intensity or material value.  A device group forwards both to every member. */
int ovr_hip_set_light(ovr_hip_renderer* r, const float direction[3], float intensity);
int ovr_hip_set_material(ovr_hip_renderer* r, float ambient, float diffuse, float specular, float shininess);
typedef struct ovr_hip_lighting {
  float direction[3];      /* the unit vector the kernels use */
  float intensity;
  float ambient, diffuse, specular, shininess;
  int32_t is_reference;    /* 1: the committed state shades exactly as the reference's literals do */
} ovr_hip_lighting;
/* the COMMITTED state: what the last frame used and the next one will, until a commit applies queued values */
int ovr_hip_get_lighting(const ovr_hip_renderer* r, ovr_hip_lighting* out);

/* Clip box (added within ABI v11 like the light and the material: new entry points and one new struct only).  The VIDI3D scene format
 * carries a `view.volume.clippingBox` next to `boundingBox`; the reference's loader drops it and its marcher has no place for it.  Here an axis-aligned box in
 * the space of grid_origin / grid_spacing cuts the volume open:
 *   lower, upper   world coordinates; lower may hold -inf and upper +inf ("open on this side").  Both NULL = no clip box.
 *   object box     per axis lo = clamp01(fmaf(lower, inv_scale, wto_p)), hi likewise from upper - the float constants that take a world position into the
 *                  volume's [0, 1] box; recomputed whenever the volume or the grid convention changes.
 *   box test       the march's test of the unit cube with lo in place of 0 and hi in place of 1 (lo = 0, hi = 1 gives the same bits); it cuts the primary
 *                  ray, EVERY shadow ray - what is cut away casts no shadow - and the schedule's block test.  Voxel taps and gradient taps read the true
 *                  voxels, also across a clip face.  lo >= hi on any axis: every ray misses (a zero frame, samples == 0).
 *                  open-volume-renderer_amd/clipping.py is this arithmetic in numpy, the normative text.
 * Queued like every setter, applied at commit; a CHANGED value resets the accumulation and voids what the layout / pipeline tuner measured, the same value
 * again resets nothing.  Until the setter is called every frame, counter and kernel is what it was without it; a clipped frame never takes the LDS-staged
 * march (the same frame, lds_rounds == 0).  EINVAL (the state stays): a NaN, lower[k] > upper[k], or exactly one pointer NULL.  A device group forwards
 * the call to every member. */
int ovr_hip_set_clip_box(ovr_hip_renderer* r, const float lower[3], const float upper[3]);
typedef struct ovr_hip_clip_box {
  int32_t enabled;                  /* 1: a clip box is committed */
  float lower[3], upper[3];         /* the world box as given (-inf / +inf without one) */
  float object_lower[3], object_upper[3]; /* what the kernels test: inside [0, 1] ((0, 0, 0), (1, 1, 1) without a clip box) */
} ovr_hip_clip_box;
/* the COMMITTED state, not the queued one */
int ovr_hip_get_clip_box(const ovr_hip_renderer* r, ovr_hip_clip_box* out);

/* Projections (added within ABI v11 like the clip box: new entry points and one new struct only).  Next to the emission-absorption march,
 * the pictures of the data itself: per ray the MAXIMUM, the MINIMUM or the MEAN of the samples the unshaded march would classify.
 *   ray      exactly the march's for the pixel sample: pixel centre, jitter, samples per pixel, normalised direction, object-space ray, the clipped box test
 *            while a clip box is committed; marched under the march's condition.
 *   steps    the reference's primary loop without its opacity condition: tx_0 = t0, ty_0 = fminf(t1, t0 + step); step i exists while ty_i > tx_i;
 *            tm_i = 0.5f * (tx_i + ty_i); s_i = the trilinear tap at fmaf(tm_i, dir, org) as the march would classify it; tx_{i+1} = ty_i,
 *            ty_{i+1} = fminf(tx_{i+1} + step, t1); n = the number of steps.
 *   modes    MAXIMUM: (m, tm*) = (-inf, 0); in step order if (s_i > m) { m = s_i; tm* = tm_i; }; v = m - a NaN is never selected, of equal samples the first
 *            counts.  MINIMUM: the same from +inf with <.  MEAN: A[i & 3] += s_i in step order from four zeros, v = ((A0 + A1) + (A2 + A3)) / (float)n, tm* = 0.
 *   pixel    not marched or n == 0: rgba = 0, layer = 0.  Otherwise rgb = clamp01(colour table at v), a = alpha table at v (the march's classification, no
 *            opacity correction), and the buffer ovr_hip_mapframe hands out as `grad` carries the PROJECTION LAYER (v, tm*, 1): the raw value for windowing on
 *            the host, the distance of the sample that set it, a hit flag.  Samples per pixel and accumulated frames combine as the march's do; everything
 *            behind the pixel - convergence estimate, sparse sampling, reconstruction, rgba8 / rgba16f, tiles, shards, device groups - works unchanged.
 *            open-volume-renderer_amd/projection.py is this arithmetic in numpy, the normative text.
 * A projection frame ignores shading mode, light, material, shadow cache, shading pipeline, LDS staging and layout choice: it reads the general layout
 * (stats.layout = 0, pipeline = 1, tuning = 0; the tuner and the adaptive-skipping probe are neither asked nor fed).  Counters: rays and active_pixels as
 * ever; samples = the steps whose voxels were fetched, skipped_samples = those whose fetch was skipped (their sum is the number of steps, always);
 * shaded_samples = shadow_samples = skipped_shadow_samples = 0.
 * Range skipping: while ovr_hip_set_empty_space_skipping(1) is committed, a MAXIMUM / MINIMUM frame skips the fetch of a step whose macrocell's value range
 * (ovr_hip_get_macrocells), widened by a derived rounding slack, proves that the sample cannot replace the running extremum - the frame, the layer and
 * samples + skipped_samples are bit for bit the non-skipping kernel's.  Unlike the majorant skip it does not depend on the transfer function.  Measured on a
 * 1024^3 f32 volume at 1920 x 1080 (profiles/r14_projection.md; the unshaded march under an all-zero alpha table over the same 274 M steps: 1.54 ms): MAXIMUM
 * 1.81 ms, MEAN 1.95 ms - slower than that march: fewer instructions, but 16-25 % more L1 misses; MAXIMUM with range skipping 0.83 ms (54 % of the steps skipped), 0.59 ms (84 %) with a
 * bright slab in front.  512^3 at 1024^2: march 0.419, MAXIMUM 0.393, MEAN 0.382, with range skipping 0.348 ms.
 * Queued, applied at commit; EVERY call resets the accumulation, like ovr_hip_set_shading.  OFF (the default) is the march, as ever: until the setter is
 * called with another mode every frame, counter and kernel is what it was without it.  EINVAL (the state stays): an unknown mode.  A device group forwards
 * the call. */
#define OVR_HIP_PROJECT_OFF 0
#define OVR_HIP_PROJECT_MAXIMUM 1
#define OVR_HIP_PROJECT_MINIMUM 2
#define OVR_HIP_PROJECT_MEAN 3
int ovr_hip_set_projection(ovr_hip_renderer* r, int32_t mode);
typedef struct ovr_hip_projection {
  int32_t mode;            /* the COMMITTED mode */
  int32_t range_skipping;  /* 1: the last projection frame ran the range-skipping kernel */
} ovr_hip_projection;
/* the COMMITTED state, not the queued one */
int ovr_hip_get_projection(const ovr_hip_renderer* r, ovr_hip_projection* out);

/* Isosurfaces (added within ABI v11 like the projections: new entry points and one new struct only).  Opaque, shaded, hard-shadowed level
 * sets of the resident volume for up to OVR_HIP_MAX_ISOVALUES isovalues, drawn in the march's place; open-volume-renderer_amd/isosurface.py is the arithmetic in
 * numpy, the normative text.  Isovalues are in the units of the projection layer's v and of ovr_hip_get_macrocells: 16-bit and float types raw, 8-bit types
 * normalised.  The setter stores them sorted ascending.
 *   ray, steps, samples   exactly the projection's (tm_i, s_i; the clipped box test while a clip box is committed).
 *   hit      side(s) = #{k : iso_k <= s} (a NaN: 0); the hit is the first step i >= 1 with side(s_{i-1}) != side(s_i).  No caps: a box face or a clip face is no
 *            surface, a ray that starts inside a solid hits where it leaves it.  Rising: the lowest isovalue crossed, falling: the highest.  The walk ends there.
 *   t*       two rounds of four points (0.2, 0.4, 0.6, 0.8 of the interval, the first sub-interval whose ends lie on different sides), then the secant, clamped to it.
 *   normal   the march's forward difference at pos* = fmaf(t*, dir, org), normalised, negated, to world space.
 *   shadow   under OVR_HIP_SHADE_FULL: 1 iff two consecutive samples of the ray pos* + t light, stepped from 1.5 steps on, differ in side - a hard shadow cast by the
 *            level sets themselves, not by the transfer function's opacity; else 0.
 *   pixel    a miss: zeros.  A hit: rgb = the colour table at the isovalue (the alpha table is not read) - as it is under OVR_HIP_SHADE_NONE, times the shade factor
 *            of the committed light and material (clamped) under GRADIENT / FULL -, a = 1; the layer (`grad`) is (isovalue, t*, 1).  Samples per pixel and accumulated
 *            frames combine as the march's do; everything behind the pixel works unchanged.
 * While n > 0 is committed frames are isosurface frames: a committed projection mode is kept but not drawn and resumes at n = 0.  Like a projection frame an
 * isosurface frame reads the general layout (stats.layout = 0, pipeline = 1, tuning = 0; tuner and adaptive-skipping probe neither asked nor fed) and ignores shadow
 * cache, pipeline, LDS staging and layout choice; it honours shading mode, light, material, clip box and ovr_hip_set_empty_space_skipping: while that is committed
 * a step's fetch is dropped when no isovalue lies in its macrocell's value range (widened by the projections' rounding slack) - on volumes of finite voxels the frame,
 * the layer, shaded_samples and samples + skipped_samples are bit for bit the non-skipping kernel's.  Counters: samples / skipped_samples = the steps walked, fetched /
 * not fetched; shaded_samples = hits; shadow_samples / skipped_shadow_samples = the shadow walks' steps; refinement and gradient taps are not counted.
 * Queued, applied at commit; EVERY call resets the accumulation, like ovr_hip_set_shading.  n = 0 (the default) is off: until the setter is called with n > 0 every
 * frame, counter and kernel is what it was without it.  EINVAL (the state stays): n < 0 or n > OVR_HIP_MAX_ISOVALUES, a null pointer with n > 0, a non-finite
 * value, two equal values.  A device group forwards the call. */
#define OVR_HIP_MAX_ISOVALUES 4
int ovr_hip_set_isosurfaces(ovr_hip_renderer* r, const float* isovalues, int32_t n);
typedef struct ovr_hip_isosurfaces {
  int32_t n;                                   /* the COMMITTED isovalues, ascending; the entries behind n are 0 */
  float isovalues[OVR_HIP_MAX_ISOVALUES];
  int32_t range_skipping;                      /* 1: the last isosurface frame ran the range-skipping kernel */
} ovr_hip_isosurfaces;
/* the COMMITTED state, not the queued one */
int ovr_hip_get_isosurfaces(const ovr_hip_renderer* r, ovr_hip_isosurfaces* out);

/* Translucent isosurfaces (added within ABI v11: new entry points and one new struct only).  Each isovalue gets an opacity alpha_k in
 * (0, 1]; a ray composites EVERY crossing front to back by the march's own recurrence until it saturates or leaves the box, and a shadow ray accumulates opacity
 * the same way: nested shells show as shells, a translucent shell casts a partial shadow.  open-volume-renderer_amd/isosurface.py stays the normative text.
 *   events     every step i >= 1 with side(s_{i-1}) != side(s_i) holds one event per isovalue crossed, in the order the ray meets them: rising from side a to
 *              b > a: k = a ... b - 1; falling to b < a: k = a - 1 ... b.  The opaque hit is the first event of the first such step.
 *   per event  t*_k by the opaque refinement from the step's own pair with iso = iso_k; pos*, normal, shade factor and shadow as for the opaque hit; c_k = the
 *              colour table at iso_k, under GRADIENT / FULL clamp01(rgb * shade).
 *   composite  from A = 0, C = 0: tr = 1 - A, C_ch = fma(tr * c_ch, alpha_k, C_ch), A = fma(tr, alpha_k, A).  The ray's first event sets the layer
 *              (iso_k, t*_k, 1).  A >= 0.9999f behind an event ends the ray there, else the walk goes on with the next step.
 *   sample     no event: zeros; else rgb = C / A per channel (un-premultiplied like the march's pixel), a = A.
 *   shadow     the opaque shadow ray and steps; A_s = fma(1 - A_s, alpha_k, A_s) over its events until A_s >= 0.9999f; shadow = A_s.
 *   counters   samples + skipped_samples = the steps walked (a step counts once however many events it holds); shaded_samples = the events composited;
 *              shadow_samples + skipped_shadow_samples = the steps of all shadow walks.
 * With every alpha_k = 1 this IS the opaque definition, bit for bit, counters included.
 * ovr_hip_set_isosurface_layers writes the queued slot of ovr_hip_set_isosurfaces, which stays and means "all opacities 1"; opacities == NULL is that call.  The
 * isovalues are stored ascending and the opacities travel with them.  Recorded and applied like the isovalues; every call resets the accumulation.  EINVAL, the
 * state kept: the cases of ovr_hip_set_isosurfaces, and an opacity that is not finite, <= 0 or > 1.  A device group forwards the call.  Until the setter is
 * called with an opacity below 1 every frame, counter and kernel is what it was: all-ones through this setter runs the opaque kernels.  ovr_hip_get_isosurfaces
 * and ovr_hip_isosurface_floats keep their meaning: the first crossing, opaque. */
int ovr_hip_set_isosurface_layers(ovr_hip_renderer* r, const float* isovalues, const float* opacities, int32_t n);
typedef struct ovr_hip_isosurface_layers {
  int32_t n;                                   /* the COMMITTED isovalues, ascending, and their opacities; the entries behind n are 0 */
  float isovalues[OVR_HIP_MAX_ISOVALUES], opacities[OVR_HIP_MAX_ISOVALUES];
  int32_t translucent, range_skipping;         /* 1: a committed opacity is below 1 - frames take the translucent kernels; 1: the last isosurface frame skipped by ranges */
} ovr_hip_isosurface_layers;
/* the COMMITTED state, not the queued one */
int ovr_hip_get_isosurface_layers(const ovr_hip_renderer* r, ovr_hip_isosurface_layers* out);

/* Ambient occlusion of the isosurface frames (added within ABI v11: new entry points and one new struct only).  While samples = K > 0 is
 * committed, every event of an isosurface frame under OVR_HIP_SHADE_GRADIENT or OVR_HIP_SHADE_FULL casts K occlusion walks into the hemisphere that faces the
 * viewer, and the event's ambient coefficient is scaled by what they find.  open-volume-renderer_amd/isosurface.py stays the normative text; float32 throughout.
 *   table      D[m][j], m = 0 ... 15, j = 0 ... K - 1: local (x, y, z), z along the normal, cosine-weighted, a sunflower spiral turned sixteen times - in float64
 *              on the host r2 = (j + 0.5) / K, phi = 2 pi (j g + m / 16) with g = 0.6180339887498949, (sqrt(r2) cos phi, sqrt(r2) sin phi, sqrt(1 - r2)), each
 *              component rounded to float32.  ovr_hip_get_ambient_occlusion_directions hands the COMMITTED table back (16 x K x 3 floats).
 *   rotation   sample k of frame frame_index (1-based) at pixel (x, y): m = ((x & 3) + 4 (y & 3) + (frame_index - 1) spp + k) & 15.
 *   normal     N = n_w if dot(n_w, dir) <= 0 else -n_w (dir: the event's primary ray; a NaN normal stays NaN, its walks miss the box).
 *   frame      s = copysign(1, N.z), a = -1 / (s + N.z), b = (N.x N.y) a, T = (1 + ((s N.x) N.x) a, s b, -(s N.x)), B = (b, s + (N.y N.y) a, -N.y).
 *   ray j      d_c = fma(x, T_c, fma(y, B_c, z N_c)) per component, not renormalised.
 *   walk       the translucent shadow walk with d_j in the light's place: (a0, a1, hit) from the (clipped) box test of pos* + t d_j from (0, FLT_MAX),
 *              a1 = fmin(a1, distance), steps by the projection's recurrence from a0 + step; A_j = fma(1 - A_j, alpha_k, A_j) over its events until
 *              A_j >= 0.9999f or its last step; the range-skipping rule is the shadow walk's; nothing is refined.
 *   shade      S = A_0 + ... + A_{K-1} in that order, O = S / (float)K; the event's shade factor takes ambient = ka * (1 - O).  O = 0 gives today's bits.
 *   counters   the AO walks' fetched steps are added to shadow_samples, their dropped steps to skipped_shadow_samples; everything else is unchanged.
 * An opaque frame runs the translucent kernels' AO twins with its all-ones opacities (the identity above makes that the opaque frame apart from the ambient
 * term).  March frames, projections and isosurface frames under OVR_HIP_SHADE_NONE never change: a committed K is kept and not used there.  samples in
 * 0 ... OVR_HIP_MAX_AO_SAMPLES, 0 (the default) = off: until the setter is called with K > 0 every frame, counter and kernel is what it was.  distance in world
 * units of t along a unit direction, finite and > 0, or +inf for the whole box; ignored (and stored as +inf) while samples == 0.  Recorded and applied like the
 * isovalues; every call resets the accumulation.  EINVAL, the state kept: samples < 0 or > 16, and with samples > 0 a distance that is NaN or <= 0.  A device
 * group forwards the call.  An occluder nearer than 1.5 steps to the event, or thinner than a step, is not seen: the shadow ray's caveat. */
#define OVR_HIP_MAX_AO_SAMPLES 16
#define OVR_HIP_AO_ROTATIONS 16
int ovr_hip_set_ambient_occlusion(ovr_hip_renderer* r, int32_t samples, float distance);
typedef struct ovr_hip_ambient_occlusion {
  int32_t samples;                             /* the COMMITTED K */
  float distance;                              /* and radius (+inf: the whole box) */
  int32_t rotations;                           /* OVR_HIP_AO_ROTATIONS */
  int32_t active;                              /* 1: the next isosurface frame takes the AO kernels - K > 0, isovalues committed, shading GRADIENT or FULL */
} ovr_hip_ambient_occlusion;
/* the COMMITTED state, not the queued one */
int ovr_hip_get_ambient_occlusion(const ovr_hip_renderer* r, ovr_hip_ambient_occlusion* out);
/* the COMMITTED direction table as the host formed it: 16 x K x 3 floats, [m][j][x, y, z] (host memory).  EINVAL: a null pointer, a capacity below that */
int ovr_hip_get_ambient_occlusion_directions(const ovr_hip_renderer* r, float* out, size_t capacity_floats);

/* Slices (added within ABI v11: new entry points and structs only): the resident volume on up to OVR_HIP_MAX_SLICES cut planes or thick
 * slabs, drawn in the march's place; open-volume-renderer_amd/slices.py is the arithmetic in numpy, the normative text.
 *   caller     per slice a world point, a world normal of any length, a thickness in world units along the normal (0: a plane; > 0: a slab centred on the
 *              plane; +inf: the whole box) and a mode, OVR_HIP_PROJECT_MAXIMUM / MINIMUM / MEAN, read only while thickness > 0.  The order given is kept.
 *   host       n = the normal normalised in float64, each component rounded to float32; c = dot(n, point) formed in float64 from the rounded n and rounded
 *              once; half = 0.5f * thickness.  ovr_hip_get_slices hands back exactly these.
 *   ray        the projection's for the pixel sample (camera kind, jitter, samples per pixel) and its box test (t0, t1, hit) - the clipped one while a clip
 *              box is committed, the orthographic rule for ignored slabs included; t is shared between world and object space.
 *   slice k    dn = fma(n.x, d.x, fma(n.y, d.y, n.z * d.z)), e = fma(n.x, o.x, fma(n.y, o.y, n.z * o.z)) - c with the world origin o and direction d.
 *              plane: ts = (-e) / dn, met iff hit, dn != 0 and t0 <= ts <= t1 (a NaN meets nothing), key ts.  slab: dn != 0: a = (-half - e) / dn,
 *              b = (half - e) / dn, swapped if a > b, ta = fmaxf(t0, a), tb = fminf(t1, b); dn == 0: (ta, tb) = (t0, t1) if |e| <= half, else not met; met iff
 *              hit and tb > ta, key ta.  thickness +inf gives (ta, tb) = (t0, t1) bit for bit: that slab's frame is the projection's of its mode.
 *   winner     the met slice with the smallest key, of equal keys the lowest index.  Only the winner is sampled: a plane by one trilinear tap at
 *              to_object(fma(ts, d, o)); a slab by the projection's steps on (ta, tb) at the committed sampling rate and its reduction of the slice's mode.  A
 *              winning slab without a step counts as not met; the next nearest slice is not tried.
 *   pixel      nothing met: rgba = 0, layer = 0.  Otherwise rgb = the projection's colour at v, clamped, a = 1 - a slice is opaque, the alpha table is not read -
 *              and the buffer mapped as `grad` carries (v, t_k, k + 1).  Samples per pixel and accumulated frames combine as the projection's; convergence,
 *              sparse sampling, reconstruction, rgba8 / rgba16f, tiles, shards and device groups work unchanged.
 *   skipping   while ovr_hip_set_empty_space_skipping(1) is committed a MAXIMUM or MINIMUM slab drops fetches by the projection's rule; the frame, the layer and
 *              samples + skipped_samples are bit for bit the non-skipping kernel's.  Planes and MEAN slabs fetch everything.
 *   counters   samples = taps fetched (a plane that is met: 1), skipped_samples = steps whose fetch was dropped, shaded / shadow counters 0, layout 0,
 *              pipeline 1, tuning 0: the tuner and the adaptive-skipping probe are neither asked nor fed.
 * While n > 0 slices are committed, frames are slice frames: committed isovalues and a committed projection mode are kept but not drawn and resume at n = 0.  Slice
 * frames ignore shading mode, light, material, shadow cache, AO, pipeline, LDS staging and layout choice; they honour camera kind, clip box, sampling rate,
 * transfer function (colours and range) and grid convention.  Queued, applied at commit; every call resets the accumulation and voids nothing else; until it is
 * called with n > 0 every frame, counter and kernel is what it was.  n = 0 or slices = NULL: off.  EINVAL (the state stays): n < 0 or n > 4, a null pointer with
 * n > 0, a non-finite point, a normal that is zero, non-finite or not normalisable, a NaN or negative thickness, with thickness > 0 a mode outside 1 ... 3.  A
 * device group forwards the call; ovr_hip_get_slices reports member 0's state.  Not done: translucent slices, lighting (the volume context around a slice: ovr_hip_set_slice_context).
 * Kernels: a plane kernel (every slice a plane: one lane per ray, one tap) and a walk kernel (a slab among them: four lanes per ray, the projection's rounds),
 * each with the clipped / orthographic twins.  Measured (tools/slice_bench.py, profiles/r21_slices.md; MI355X, 1024^3 f32, 1920 x 1080, kernel_ms): one axial plane
 * 0.046, three orthogonal planes 0.050, one oblique plane 0.045, a 32-voxel oblique MAXIMUM slab 0.164 (0.162 with range skipping,
 * 33 % of the fetches dropped), the MEAN slab 0.164, the +inf MAXIMUM slab 1.669 beside the MAXIMUM projection frame's 1.864 and the unshaded
 * march's 1.343 on the same camera. */
#define OVR_HIP_MAX_SLICES 4
typedef struct ovr_hip_slice { float point[3], normal[3], thickness; int32_t mode; } ovr_hip_slice;
int ovr_hip_set_slices(ovr_hip_renderer* r, const ovr_hip_slice* slices, int32_t n);
typedef struct ovr_hip_slices {
  int32_t n;                                   /* the COMMITTED slices, in the order given */
  struct { float normal[3], c, thickness; int32_t mode; } slice[OVR_HIP_MAX_SLICES];
  int32_t walks;                               /* 1: a slab is among them - the frame takes the walk kernel */
  int32_t range_skipping;                      /* 1: the last slice frame ran the range-skipping kernel */
} ovr_hip_slices;
/* the COMMITTED state, not the queued one */
int ovr_hip_get_slices(const ovr_hip_renderer* r, ovr_hip_slices* out);

/* Slice context (added within ABI v11: new entry points and one new struct only): the volume marched IN FRONT of the cut planes.  A context
 * frame is a slice frame in which the unshaded emission-absorption march runs from the ray's entry into the box up to the winning slice; the opaque slice is
 * composited behind it.  open-volume-renderer_amd/slice_context.py is the arithmetic in numpy, the normative text.  Per pixel sample:
 *   ray, stage the slice frame's: (t0, t1, hit) and the winner (k, key, ta, tb), met under its rule (a winning slab without a step counts as not met); a ray that is
 *              not hit gives zeros.
 *   cut        tc = key if a slice is met, else t1.
 *   context    the march's primary loop under OVR_HIP_SHADE_NONE with tc in t1's place, operation for operation: alpha = 0, C = 0, tx = t0,
 *              ty = fminf(tc, t0 + step); while ty > tx and alpha < 0.9999f: tm = 0.5f * (tx + ty), the tap at to_object(fma(tm, d, o)), the march's classification
 *              (rgb, a_tf), a = opacity_correction(a_tf, base, ty - tx), a' = a * opacity_scale, tr = 1 - alpha, C_ch = fma(tr * clamp01(rgb_ch), a', C_ch),
 *              alpha = fma(tr, a', alpha), tx = ty, ty = fminf(tx + step, tc).
 *   slice      composited iff one is met and alpha < 0.9999f (the loop's own condition: a saturated ray neither taps a plane nor walks a slab): v the slice
 *              frame's, c = its clamped colour at v, tr = 1 - alpha, C_ch = fma(tr * c_ch, 1, C_ch), alpha = fma(tr, 1, alpha); the layer (the buffer mapped as
 *              `grad`) is (v, t_k, k + 1) when the slice was composited, else zeros.
 *   sample     a = alpha, rgb = C / a per channel if a > 0, else 0: the march's un-premultiplied pixel.  Samples per pixel and accumulated frames as the slice frame's.
 *   counters   samples = context steps fetched + the composited winner's fetched taps; shaded_samples = context steps with a' > 0 (what the march counts under
 *              SHADE_NONE); skipped_samples 0, shadow counters 0, layout 0, pipeline 1, tuning 0.
 * Consequences, each exact: with no slice met on a ray and scale 1 the sample is the SHADE_NONE march's bit for bit (a frame whose slices no ray meets IS the
 * march frame, counters included); with an all-zero alpha table or scale 0 frame and layer are the slice frame's bit for bit; mode OFF is the slice frame, kernel
 * included.  A context frame honours what a slice frame honours - camera kind, clip box, sampling rate, grid convention, the transfer function's colours and
 * range, samples per pixel, jitter, everything behind the pixel - and the transfer function's alpha table.  THE CONTEXT IS ALWAYS UNSHADED: the shading mode is
 * ignored, as are light, material, shadow cache, ambient occlusion, pipeline, LDS staging and layout choice; it reads the general layout; the tuner and the
 * adaptive-skipping probe are neither asked nor fed.  While empty-space skipping is committed a context frame still fetches every step, a slab inside it is not
 * range-skipped and ovr_hip_get_slices().range_skipping reads 0.
 * Queued, applied at commit, recorded with the other frame kinds: every call resets the accumulation and voids nothing else; until it is called with a mode other
 * than OFF every frame, counter and kernel is what it was.  The mode is kept while no slice is committed and takes effect when n > 0.  opacity_scale is ignored,
 * and stored as 1, in mode OFF.  EINVAL (the state stays): an unknown mode; in mode FRONT an opacity_scale that is NaN, negative or above 1.  A device group
 * forwards the call; ovr_hip_get_slice_context reports member 0's state.
 * Not done: a shaded context, majorant (empty-space) skipping of the context march, range skipping of a slab under context, translucent slices.
 * Kernel: slice_context_kernel, one per general voxel type, addressing mode and camera, on the clipped box test alone (the unit box without a clip box) - four
 * lanes per ray, rounds of 16 steps, the transfer function in LDS.  Measured: tools/slice_context_bench.py, profiles/r22_slice_context.md. */
#define OVR_HIP_SLICE_CONTEXT_OFF 0
#define OVR_HIP_SLICE_CONTEXT_FRONT 1
int ovr_hip_set_slice_context(ovr_hip_renderer* r, int32_t mode, float opacity_scale);
typedef struct ovr_hip_slice_context {
  int32_t mode;          /* COMMITTED */
  float opacity_scale;
  int32_t active;        /* 1: the next frame is a context frame - mode FRONT and n > 0 slices committed */
} ovr_hip_slice_context;
int ovr_hip_get_slice_context(const ovr_hip_renderer* r, ovr_hip_slice_context* out);

/* Isosurface context (added within ABI v11: new entry points and one new struct only): the volume marched AROUND the level sets.  In a
 * context frame ONE walk both composites the unshaded emission-absorption march and finds, shades and composites every crossing of the committed isovalues, each in
 * its place along the ray: a bone surface inside translucent soft tissue.  open-volume-renderer_amd/isosurface_context.py is the arithmetic in numpy, the normative
 * text.  Per pixel sample, float32 throughout:
 *   ray, steps the isosurface frame's: (t0, t1, hit) of the (clipped) box test, tx_0 = t0, ty_0 = fminf(t1, t0 + step), tm_i = 0.5f * (tx_i + ty_i), tx_{i+1} = ty_i,
 *              ty_{i+1} = fminf(tx_{i+1} + step, t1); s_i the tap at to_object(fma(tm_i, d, o)).
 *   state      A = 0, C = 0, layer unset; step i exists while ty_i > tx_i and A < 0.9999f - the march's loop condition, tested before every step.
 *   step i     1. events, if i >= 1 and side(s_{i-1}) != side(s_i): the translucent frame's events of the step in its order (ovr_hip_set_isosurface_layers), each with
 *              its t*_k, pos*, normal, shade factor and colour c_k, composited by its expressions with the isovalue's own opacity alpha_k (the scale does not touch
 *              it): tr = 1 - A, C_ch = fma(tr * c_ch, alpha_k, C_ch), A = fma(tr, alpha_k, A).  The ray's first event sets the layer (iso_k, t*_k, 1).
 *              A >= 0.9999f behind an event ends the ray there: later events of the step and the step's own volume sample are not taken.
 *              2. the volume sample, the march's under OVR_HIP_SHADE_NONE, operation for operation: (rgb, a_tf) the march's classification of s_i,
 *              a = opacity_correction(a_tf, base, ty_i - tx_i), a' = a * opacity_scale, tr = 1 - A, C_ch = fma(tr * clamp01(rgb_ch), a', C_ch), A = fma(tr, a', A).
 *              (The surface of step i lies between tm_{i-1} and tm_i, in front of sample i: hence this order.)
 *   sample     a = A, rgb = C / A per channel if A > 0, else 0.  Samples per pixel and accumulated frames as the isosurface frame's; everything behind the pixel
 *              works unchanged.
 *   shading    the events honour the committed shading mode, light and material exactly as an isosurface frame's do; under OVR_HIP_SHADE_FULL the shadow ray is the
 *              translucent frame's, cast by the level sets alone with their opacities.
 *   counters   samples = steps walked (every step fetches: a context frame never range-skips, on the primary walk or on a shadow walk); skipped_samples =
 *              skipped_shadow_samples = 0; shaded_samples = events composited + volume samples composited with a' > 0; shadow_samples = the steps of all shadow
 *              walks; layout 0, pipeline 1, tuning 0 (the tuner and the adaptive-skipping probe are neither asked nor fed).
 * Consequences, each exact (x * 1.0f, fma(tr, 0, A) and fma(p, 0, C) with finite p are exact): with no crossing on any ray and scale 1 frame and counters are the
 * SHADE_NONE march's bit for bit; with an all-zero alpha table or scale 0 on a volume of finite voxels frame, layer, shaded_samples and the shadow steps are the
 * translucent isosurface frame's (by its own identity the opaque frame's too) bit for bit, and samples equals that frame's samples + skipped_samples; mode OFF is
 * the isosurface frame, kernel included.
 * Queued, applied at commit, recorded with the other frame kinds: every call resets the accumulation and voids nothing else; until it is called with a mode other
 * than OFF every frame, counter and kernel is what it was.  The mode is kept while no isovalue is committed; `active` = mode VOLUME, n > 0 isovalues committed and no
 * slices committed (slices keep their precedence).  opacity_scale is ignored, and stored as 1, in mode OFF.  EINVAL (the state stays): an unknown mode; in mode
 * VOLUME an opacity_scale that is NaN, negative or above 1.  A device group forwards the call; ovr_hip_get_isosurface_context reports member 0's committed state.
 * Not done: a shaded context (THE CONTEXT IS ALWAYS UNSHADED); volume shadows on the surfaces (the volume casts no shadow on a surface); ambient occlusion (a
 * committed ovr_hip_set_ambient_occlusion is kept and not used); range and majorant skipping.
 * Kernel: isosurface_context_kernel, one per general voxel type, addressing mode, shading mode and camera, on the clipped box test alone (the unit box without a
 * clip box) - four lanes per ray, rounds of 16 steps that end at their first crossing step, the transfer function in LDS.  Measured:
 * tools/isosurface_context_bench.py, profiles/r23_isosurface_context.md. */
#define OVR_HIP_ISO_CONTEXT_OFF 0
#define OVR_HIP_ISO_CONTEXT_VOLUME 1
int ovr_hip_set_isosurface_context(ovr_hip_renderer* r, int32_t mode, float opacity_scale);
typedef struct ovr_hip_isosurface_context {
  int32_t mode;          /* COMMITTED */
  float opacity_scale;
  int32_t active;        /* 1: the next frame is a context frame - mode VOLUME, n > 0 isovalues and no slices committed */
} ovr_hip_isosurface_context;
int ovr_hip_get_isosurface_context(const ovr_hip_renderer* r, ovr_hip_isosurface_context* out);

/* Pre-integrated classification (added within ABI v11: new entry points and one new struct only): the unshaded march in which every SEGMENT
 * between two consecutive samples is classified by the integral of the transfer function over the values the segment spans, instead of one tap at the middle of
 * the step looked up once.  A feature of the transfer function narrower than the data's change over one step is then neither hit nor missed by luck.
 * open-volume-renderer_amd/preintegration.py is the arithmetic in numpy, the normative text.
 * The node table (host, float64, rounded once to float32): M = S * max(n_alpha - 1, n_color - 1, 1) + 1 nodes at u_j = j / (M - 1), S the largest of 4, 2, 1 whose
 * table fits the frame's LDS budget beside axis tables and transfer function (a third of a CU's 160 KiB: three workgroups per CU); a_j = clamp01 of the alpha
 * table's nodal lerp at u_j, c_j = clamp01 per channel of the colour table's, tau_j = -log2(1 - min(a_j, 1 - 2^-24)); T_j and K_j (rgb) the cumulative trapezoid
 * sums of tau and tau * c over u; a node is (T, Kr, Kg, Kb), and the table carries one more entry, a copy of the last.
 * Per pixel sample - ray, box test, t0, t1, step = 1 / rate and base = 1 as in the unshaded march, all float32, every fma explicit:
 *   alpha = 0, C = 0, tx = t0, ty = fminf(t1, t0 + step); uf = tf_coord(the tap at to_object(fma(tx, d, o)))      - the entry tap
 *   while ty > tx and alpha < 0.9999f:
 *     ub = tf_coord(the tap at to_object(fma(ty, d, o)))                                                          - ONE tap per segment
 *     du = ub - uf, dt = ty - tx, adj = base * dt
 *     if fabsf(du) * (M - 1) < 1:  um = 0.5f * (uf + ub); a = opacity_correction(tf_alpha(um), adj); c = clamp01(tf_color(um))   - the march's own classification
 *     else:  (Tf, Kf), (Tb, Kb) = the node lerp at uf, ub (i0 = (int)(u * (M - 1)), its fraction, the lerp of nodes i0 and i0 + 1); Td = Tb - Tf;
 *            a = clamp01(1 - exp2(-((Td / du) * adj))); c = clamp01((Kb - Kf) / Td) per channel if Td != 0, else 0
 *     tr = 1 - alpha; C_ch = fma(tr * c_ch, a, C_ch); alpha = fma(tr, a, alpha); tx = ty, ty = fminf(tx + step, t1), uf = ub
 *   the pixel is the march's un-premultiplied sample.  samples counts the segments taken - the entry tap is NOT counted -, shaded_samples the segments with a > 0;
 *   skipped_samples 0, shadow counters 0, layout 0, pipeline 1, tuning 0; the gradient layer is zero.
 * Consequences: over a constant volume every segment takes the first branch at um = uf and the frame is the SHADE_NONE march's bit for bit, counters included;
 * along an axis-parallel ray through a linear ramp Td / du * dt telescopes, so alpha does not depend on the sampling rate (up to rounding, below 0.9999).
 * exp2 is v_exp_f32 in the product and the machine-independent det_exp2 in the model and the exact-parity build; both divisions are IEEE divides everywhere.
 * A frame is pre-integrated iff the committed frame is the march (no slices, isovalues or projection), the committed shading mode is OVR_HIP_SHADE_NONE and the mode is
 * SEGMENTS; under GRADIENT or FULL shading the mode is kept and not drawn - the frame is the ordinary shaded march.  A pre-integrated frame honours camera kind, clip
 * box, sampling rate, transfer function (tables and range), grid convention, samples per pixel, jitter, accumulation, sparse sampling, image shards and device
 * groups.  It fetches every step (no empty-space-skipping twin), ignores LDS staging and the layout choice (it reads the general layout), and neither asks nor feeds
 * the tuner.  A transfer function whose node table does not fit the LDS budget at S = 1 makes the frame fail with EINVAL, like one too large for tf staging.
 * Queued, applied at commit, recorded with the other frame kinds: every call resets the accumulation and voids nothing else; until it is called with a mode other
 * than OFF every frame, counter and kernel is what it was.  EINVAL (the state stays): an unknown mode.  A device group forwards the call;
 * ovr_hip_get_preintegration reports member 0's state.
 * Not done: a shaded pre-integrated march (GRADIENT / FULL), pre-integration of the two contexts' marches, majorant (empty-space) skipping of the pre-integrated
 * march, reciprocal multiplies in the divisions' place, the mode walk of tests/mode_walk.py over the new kind.
 * Kernel: preintegrated_kernel, one per general voxel type, addressing mode and camera, on the clipped box test alone - four lanes per ray, rounds of 16
 * segments, one tap and one node lookup per segment, transfer function and node table in LDS.  Measured: tools/preintegration_bench.py,
 * profiles/r24_preintegration.md. */
#define OVR_HIP_PREINTEGRATION_OFF 0
#define OVR_HIP_PREINTEGRATION_SEGMENTS 1
int ovr_hip_set_preintegration(ovr_hip_renderer* r, int32_t mode);
typedef struct ovr_hip_preintegration {
  int32_t mode;        /* COMMITTED */
  int32_t active;      /* 1: the next frame is a pre-integrated frame - mode SEGMENTS, the march committed, shading NONE */
  int32_t nodes;       /* M of the node table built last; 0 until a pre-integrated frame or ovr_hip_get_preintegration_tables built one for the committed tables */
  int32_t subdivision; /* its S */
} ovr_hip_preintegration;
int ovr_hip_get_preintegration(const ovr_hip_renderer* r, ovr_hip_preintegration* out);
/* the float32 node table the frames read: 4 floats per node (T, Kr, Kg, Kb); builds it if stale.  *n_nodes = M; nodes_host (optional) receives M nodes and must
 * hold capacity_nodes >= M of them.  ESTATE without a volume or a committed transfer function; EINVAL: a null renderer or n_nodes, too small a capacity, a table that
 * does not fit the LDS budget */
int ovr_hip_get_preintegration_tables(ovr_hip_renderer* r, float* nodes_host, size_t capacity_nodes, int32_t* n_nodes);

/* Gradient opacity (added within ABI v11: new entry points and one new struct only): the march in which the transfer function's opacity
 * of every sample is weighted by the magnitude of the local gradient (Levoy 1988; VTK's "gradient opacity"), so that the inside of a homogeneous material fades
 * and its boundaries stay - what a 1-D table cannot tell apart.  The reference has no such control: like the clip box, the definition is this project's.
 * open-volume-renderer_amd/gradient_opacity.py is the arithmetic in numpy, the normative text.
 * State: (mode, lo, hi), lo < hi, both finite, lo may be negative; in mode OFF the thresholds are ignored and stored as (0, 1).  inv_ramp = 1.f / (hi - lo), once,
 * in float32, on the host.
 * Per pixel sample the loop is the unshaded march's - ray, box test, t0, t1, step = 1 / rate, base = 1, all float32, every fma explicit.  After the tap s at the
 * object position po and a_tf, rgb from the march's classification:
 *   if a_tf > 0:                                  - otherwise no gradient is fetched: a_tf * w is 0 whatever w
 *     d_k = -g_k if po_k + g_k > 1 else g_k       - g_k = 1 / n_k (vertex-centred: 1 / (n_k - 1)): the shading's forward difference
 *     G_k = (tap(po + d_k e_k) - s) / d_k         - the product multiplies with the stored reciprocal, DESIGN.md section 3's existing approximated place
 *     W_k = G_k * inv_scale_k                     - the world gradient, sample units per world length
 *     m   = sqrtf(fma(Wx, Wx, fma(Wy, Wy, Wz * Wz))) * tf_scale    - tf_scale: the transfer-function coordinate's scale, 0 for a degenerate range
 *     w   = clamp01((m - lo) * inv_ramp);  a_tf = a_tf * w
 *   a = opacity_correction(a_tf, base * (ty - tx))
 * m is "fraction of the transfer function's range per world unit length" and does not depend on the voxel type; sqrtf is correctly rounded in both builds.
 * Under shading NONE the composite is the march's and the gradient layer zero.  Under shading GRADIENT a step with a > 0 uses the same G for the light:
 * n_o = -normalize(G), n_w = normalize(n_o * inv_scale), the camera normal as the shaded march forms it, shade = ka + light(n_w) with the committed material and
 * light, C = fma(tr * clamp01(rgb * shade), a, C), and the gradient layer accumulates fma(tr * clamp01(n_c), a, .): operation for operation the GRADIENT-shaded
 * march.  Counters: samples = steps taken, shaded_samples = steps with a > 0; shadow and skipped counters 0, layout 0, pipeline 1, tuning 0.
 * Consequences: with (lo, hi) = (-1, 0) w == 1 for every m >= 0 and the frame is the same state's OFF frame bit for bit, under NONE and GRADIENT, counters and
 * gradient layer included; over a constant volume with lo >= 0 the frame is zero with shaded_samples == 0 and the march's samples; on a linear ramp with hi at
 * most the ramp's slope (in m's units) w == 1 and the frame is the OFF frame bit for bit; where every w is exactly 0.5 the frame is the OFF frame's under the
 * alpha table times 0.5.
 * A frame is a gradient-opacity frame iff the committed frame is the march (no slices, isovalues or projection), the mode is RAMP, the committed shading mode is
 * OVR_HIP_SHADE_NONE or OVR_HIP_SHADE_GRADIENT, and the frame is not a pre-integrated one; under FULL shading, slices, isovalues, a projection or an active
 * pre-integration the mode is kept and not drawn.  Such a frame honours camera kind, clip box, sampling rate, transfer function, grid convention, samples per
 * pixel, jitter, accumulation, sparse sampling, image shards and device groups.  It fetches every step (no empty-space-skipping twin), reads the general layout,
 * ignores LDS staging and neither asks nor feeds the tuner.
 * Queued, applied at commit, recorded with the other frame kinds: every call resets the accumulation and voids nothing else; until it is called with mode RAMP
 * every frame, counter and kernel is what it was.  EINVAL (the state stays): an unknown mode, a non-finite threshold, lo >= hi in mode RAMP.  A device group
 * forwards the call; ovr_hip_get_gradient_opacity reports member 0's state.
 * Not done: FULL shading and shadow rays whose opacity is gradient-weighted, a 2-D (value x gradient) table or a piecewise weight, gradient opacity inside the
 * two contexts or the pre-integrated march, empty-space skipping of the new march, a scene-file field, the mode walk of tests/mode_walk.py over the new kind.
 * Kernel: gradient_opacity_kernel, one per general voxel type, addressing mode, shading mode (NONE, GRADIENT) and camera, on the clipped box test alone - four
 * lanes per ray, rounds of 16 steps, the three gradient taps of a step behind a wave-uniform ballot on a_tf > 0, transfer function in LDS.  Measured:
 * tools/gradient_opacity_bench.py, DESIGN.md section 25. */
#define OVR_HIP_GRADIENT_OPACITY_OFF 0
#define OVR_HIP_GRADIENT_OPACITY_RAMP 1
int ovr_hip_set_gradient_opacity(ovr_hip_renderer* r, int32_t mode, float lo, float hi);
typedef struct ovr_hip_gradient_opacity {
  int32_t mode;    /* COMMITTED */
  int32_t active;  /* 1: the next frame is a gradient-opacity frame - mode RAMP, the march committed, shading NONE or GRADIENT, no active pre-integration */
  float lo, hi;    /* (0, 1) in mode OFF */
  float inv_ramp;  /* 1.f / (hi - lo) as the kernels multiply with it */
} ovr_hip_gradient_opacity;
int ovr_hip_get_gradient_opacity(const ovr_hip_renderer* r, ovr_hip_gradient_opacity* out);

/* Depth limit (added within ABI v11: new entry points and one new struct only): the march that ends every ray of a pixel on a ray
 * parameter the caller hands in - the distance of the opaque geometry (a mesh, an instrument, a bounding frame, another renderer's picture) the application drew
 * at that pixel - so that the frame is what lies IN FRONT of that geometry and can be blended over the caller's picture (rgb * a + own * (1 - a)).  VTK and
 * ParaView end rays at the depth buffer, OSPRay takes a map_maxDepth texture; the reference has no such control: like the clip box, the definition is this
 * project's.  open-volume-renderer_amd/max_depth.py is the arithmetic in numpy, the normative text.
 * depth: width * height float32 values in the frame's own pixel order - the order of ovr_hip_mapframe's rgba: the value of pixel (ix, iy) is at ix + iy * width.
 * UNITS: the march's own t - WORLD LENGTH ALONG THE NORMALISED RAY DIRECTION FROM THE RAY'S ORIGIN.  Under the perspective camera that is the Euclidean distance
 * from the camera position; it is not a planar z and not a z-buffer value (max_depth.ray_distance_from_planar converts an eye-space z).  Under the orthographic
 * camera it is the distance from the image plane through `from`: the planar depth of section 18.
 * The renderer keeps its own device copy: depth (host or device memory, mem_kind) is not referenced after the call returns.  depth == NULL switches the limit off
 * (the other arguments are not read).
 * Per pixel sample of pixel (ix, iy), with (t0, t1, hit) as the march forms them:
 *   z = depth[ix + iy * width]        - every sample of a pixel (spp > 1, pixel jitter) takes the pixel's value
 *   limited = z < +inf                - false for +inf and for NaN: no surface at this pixel
 *   tc = limited ? fminf(t1, z) : t1
 * and from there the loop is the march's with tc in t1's place, operation for operation: under shading NONE slice_context.py's step 3 with scale 1, under
 * shading GRADIENT the gradient-shaded step of gradient_opacity.py with the opacity left unweighted.  The last step ends on tc: ty = fminf(tx + step, tc),
 * dt = ty - tx goes through the opacity correction; a step of length 0 is not taken; z <= t0 (any negative value, -inf) takes no step.  Nothing is composited
 * behind the cut: the pixel is the march's un-premultiplied (rgb, alpha) of what lies in front of the surface.  The gradient layer is zero under NONE and the
 * march's under GRADIENT.  Counters: samples = steps taken, shaded_samples = steps with a > 0; shadow and skipped counters 0, layout 0, pipeline 1, tuning 0.
 * Consequences: an image of +inf, of NaN or of values >= every t1 gives the same state's frame without the limit bit for bit, counters and gradient layer
 * included; depth = the clipped march's t1 (0 where the clipped ray misses) under a clip box that removes only the far side gives the clipped frame.
 * A frame is a depth-limited frame iff the committed frame is the march (no slices, isovalues or projection), an image is committed, the committed shading mode
 * is OVR_HIP_SHADE_NONE or OVR_HIP_SHADE_GRADIENT, neither pre-integration nor gradient opacity is active (their own rules and `active` flags stay what they
 * are), and the image's size equals the committed framebuffer size.  Otherwise the image is kept and not drawn.  Such a frame honours camera kind, clip box,
 * sampling rate, transfer function, grid convention, samples per pixel, jitter, accumulation, sparse sampling, image shards and device groups (every member
 * holds the whole image and indexes it by the full frame's pixel index).  It fetches every step, reads the general layout, ignores LDS staging and neither asks
 * nor feeds the tuner.
 * Queued, applied at commit, recorded with the other frame kinds: every call resets the accumulation and voids nothing else - every call with an image counts as
 * a change, contents are not compared; until it is called with an image every frame, counter and kernel is what it was.  The frame in flight is resolved before
 * the image is copied.  EINVAL, checked before anything changes (the state stays): a bad mem_kind, width or height < 1, width x height beyond 2^31 - 1 pixels.
 * Not done: FULL shading and shadow rays that see the surface; the limit on projections, isosurfaces, slices, the two contexts, pre-integration and gradient
 * opacity; compositing a colour inside the renderer; empty-space skipping, the tuner and the layout choice for the new kernel; a depth OUTPUT layer; the mode walk
 * of tests/mode_walk.py over the new kind.
 * Kernel: max_depth_kernel, one per general voxel type, addressing mode, shading mode (NONE, GRADIENT) and camera, on the clipped box test alone - four lanes
 * per ray, rounds of 16 steps, one depth load per pixel, transfer function in LDS.  Measured: tools/max_depth_bench.py, DESIGN.md section 26. */
#define OVR_HIP_MAX_DEPTH_OFF 0
#define OVR_HIP_MAX_DEPTH_ON 1
int ovr_hip_set_max_depth(ovr_hip_renderer* r, const float* depth, int mem_kind, int32_t width, int32_t height);
typedef struct ovr_hip_max_depth {
  int32_t mode;          /* COMMITTED: OVR_HIP_MAX_DEPTH_ON while an image is held */
  int32_t active;        /* 1: the next frame is a depth-limited frame - see above */
  int32_t width, height; /* of the committed image; 0 in mode OFF */
} ovr_hip_max_depth;
int ovr_hip_get_max_depth(const ovr_hip_renderer* r, ovr_hip_max_depth* out);
/* the committed image, read back: width x height floats into depth_host (capacity_floats of them; EINVAL where that is too few); width and height are always
 * written (0 in mode OFF, where nothing is copied); depth_host == NULL asks for the size alone */
int ovr_hip_get_max_depth_values(ovr_hip_renderer* r, float* depth_host, size_t capacity_floats, int32_t* width, int32_t* height);

/* Depth layer (added within ABI v11: new entry points and one new struct only): the counterpart of the depth limit - the march says
 * WHERE along each ray its picture is, so that an application can write the volume into its z-buffer, pick the structure under the cursor, reproject a frame,
 * or hand one volume's depth to a second renderer as that renderer's limit.  VTK, ParaView and OSPRay hand a depth out with the picture; the reference has no
 * such output: like the clip box and the depth limit, the definition is this project's.  open-volume-renderer_amd/depth_output.py is the arithmetic in numpy,
 * the normative text.
 * Per pixel sample, with (t0, t1, hit), step and the cut tc exactly as the depth limit forms them (tc = t1 when no limit applies), the march's loop with four
 * more values, S = 0, d = 0, reached = false, k = 0.  Every step that is taken forms tr = 1 - alpha and alpha = fma(tr, a, alpha) as before, and also
 *   S = fma(tr * tm, a, S)                         - tm the step's midpoint: a colour channel whose colour is tm
 *   if (!reached && a > 0 && alpha >= threshold)   - alpha AFTER the step
 *     reached = true, d = ty, k = steps taken so far, this one included        - ty is the BACK end of the crossing step
 * Nothing else of the loop changes: rgb, alpha, the termination test and the counters are the march's operation for operation.  The pixel sample's layer is
 * (reached ? d : 0, S, reached ? 1 : 0); samples per pixel sum and are scaled by 1 / spp as the march's gradient layer is, and like that layer the one
 * ovr_hip_mapframe hands out is the LAST frame's (the layer is not accumulated; rgba is).  From a frame:
 *   threshold depth             = layer[0] / layer[2] where layer[2] > 0
 *   alpha-weighted mean depth   = layer[1] / rgba[3]  where rgba[3] > 0      (rgba[3] is the sum of tr * a exactly; of the same frame: without accumulation)
 *   layer[2]                    = the share of the pixel's samples that reached the threshold
 * (depth_output.resolve; +inf - the depth limit's "no surface" - where a depth is undefined).  UNITS: every depth is the march's own t, exactly what
 * ovr_hip_set_max_depth takes (depth_output.planar_from_ray_distance converts to an eye-space z).
 * threshold: a float in (0, 0.9999f].  The smallest positive normal float gives the back end of the first step with opacity, 0.5 the "median" surface; above
 * the march's early-termination literal a crossing could only happen by overshoot, and is refused.  ty is recorded and not tm: handed back as a depth limit,
 * fminf(tx + step, d) == d on the crossing step, and the limited march takes exactly the same k steps with the same bits.
 * A frame is a depth frame iff the committed frame is the march (no slices, isovalues or projection), the mode is ON, the committed shading mode is
 * OVR_HIP_SHADE_NONE or OVR_HIP_SHADE_GRADIENT, and neither pre-integration nor gradient opacity is active (their own rules and `active` flags stay what they
 * are).  Otherwise the setting is kept and not drawn.  A depth frame's rgba and counters are the march's bit for bit; the layer replaces the gradient layer,
 * under GRADIENT too (as projections do).  A committed depth image of the framebuffer's size is applied by the depth frame - same tc, same load, one per pixel -
 * and `limited` says so; without one the kernel takes z = +inf without a load.
 * Queued, applied at commit, recorded with the other frame kinds: every call resets the accumulation and voids nothing else.  Until it is called with ON every
 * frame, counter, kernel and getter is what it was.  EINVAL, with the state kept: an unknown mode; mode ON with threshold NaN, <= 0 or > 0.9999f.  A device
 * group forwards the call.
 * Not done: FULL shading; the layer on projections, isosurfaces, slices, the two contexts, pre-integration and gradient opacity (projection and isosurface
 * frames carry a distance of their own); accumulating the layer over frames; empty-space skipping, the tuner and the layout choice for the new kernel; the mode
 * walk of tests/mode_walk.py over the new kind.
 * Kernel: depth_output_kernel, the depth-limited kernel's variants and frame shell with S, the step count and the crossing in the recurrence.  Measured:
 * tools/depth_output_bench.py, DESIGN.md section 27. */
#define OVR_HIP_DEPTH_OUTPUT_OFF 0
#define OVR_HIP_DEPTH_OUTPUT_ON 1
int ovr_hip_set_depth_output(ovr_hip_renderer* r, int32_t mode, float threshold);
typedef struct ovr_hip_depth_output {
  int32_t mode;      /* COMMITTED */
  int32_t active;    /* 1: the next frame is a depth frame - see above */
  int32_t limited;   /* 1: ... and it applies the committed depth image */
  float threshold;   /* COMMITTED; 0 in mode OFF */
} ovr_hip_depth_output;
int ovr_hip_get_depth_output(const ovr_hip_renderer* r, ovr_hip_depth_output* out);

/* Shadow cache (added within ABI v11 like the clip box: new entry points and one new struct only).  Full shading marches one shadow ray
 * per shaded sample towards ONE directional light; volume, transfer function and light are static while a camera orbits, so the shadow term is a
 * view-independent scalar field.  It can be computed once on a lattice and read back with one trilinear tap:
 *   lattice   over the volume's unit cube; per axis a of dim_a voxels and `cell_voxels` >= 1: N_a = ceil(dim_a / cell) + 1 nodes, node i at
 *             u_i = (float)i / (float)(N_a - 1), world position fmaf(u_i, spacing_a * ext_a, origin_a); N_x * N_y * N_z floats, x fastest.
 *   node      what the shadow march of the marched frame returns from the node's position: the committed light direction, sampling rate, transfer function,
 *             grid convention and clip box, early termination included.
 *   lookup    for a shaded sample at the object position po: g_a = clamp01(po_a) * (N_a - 1), i_a = min(floor(g_a), N_a - 2), f_a = g_a - i_a, trilinear
 *             interpolation with lerp(a, b, f) = fmaf(f, b - a, a) along x, then y, then z; not clamped.  The shade expression is unchanged.
 *             open-volume-renderer_amd/shadow_cache.py is this arithmetic in numpy, the normative text.
 *   modes     MARCHED (default): the shadow march, as ever - no buffer, no launch, the same kernels.  CACHED: frames whose committed shading is
 *             OVR_HIP_SHADE_FULL take the shadow term from the lattice; it is (re)built on the renderer's stream before the first such frame after a change
 *             of volume (ovr_hip_set_volume, ovr_hip_update_volume: a whole rebuild), transfer function, sampling rate, light direction, clip box, grid
 *             convention, cell or mode - and of nothing else (camera, framebuffer, samples per pixel, jitter, material, light intensity, ...).  SUPPLIED: the
 *             same lookup on a lattice the caller uploaded (ovr_hip_set_shadow_cache_values), e.g. an occlusion volume computed elsewhere; never rebuilt.
 * The approximation error depends on the cell size relative to the size of what casts the shadows (DESIGN.md section 14 has a table); it is a quality / speed
 * control.  Frames with shading NONE or GRADIENT build nothing and are untouched.  A cached frame reports shadow_samples == 0 and
 * skipped_shadow_samples == 0; the build's time and iterations are reported by ovr_hip_get_shadow_cache, never in kernel_ms.
 * Queued, applied at commit; cell_voxels 0 = the default (4).  A changed mode or cell resets the accumulation and voids the tuner's measurement, the same value
 * again resets nothing.  EINVAL (the state stays): an unknown mode, cell_voxels < 0, a lattice of more than 2^31 - 1 nodes for the resident volume.  ESTATE:
 * SUPPLIED without uploaded values.  A device group forwards the call; every member builds its own, identical lattice - also a renderer that draws an image
 * shard builds the whole lattice (it is view-independent): that work is redundant across ranks. */
#define OVR_HIP_SHADOWS_MARCHED 0
#define OVR_HIP_SHADOWS_CACHED 1
#define OVR_HIP_SHADOWS_SUPPLIED 2
int ovr_hip_set_shadow_cache(ovr_hip_renderer* r, int32_t mode, int32_t cell_voxels);
/* the lattice of mode SUPPLIED: dims[k] >= 2 nodes per axis spanning the unit cube, dims[0] * dims[1] * dims[2] finite floats, x fastest (host or device memory);
 * copied at once, kept until a commit changes the mode away from SUPPLIED.  EINVAL (the state stays): a null pointer, a bad mem_kind, a dims < 2, more than
 * 2^31 - 1 nodes, a value that is not finite.  EDEVICE: the allocation failed - the previous values stay. */
int ovr_hip_set_shadow_cache_values(ovr_hip_renderer* r, const float* values, int mem_kind, const int32_t dims[3]);
typedef struct ovr_hip_shadow_cache {
  int32_t mode, cell;             /* the COMMITTED mode and cell size in voxels */
  int32_t dims[3];                /* nodes per axis of the lattice the next cached frame reads (0 without one) */
  int32_t valid;                  /* 1: that lattice is current - built since the last change, or supplied */
  uint64_t builds;                /* builds since the renderer was created */
  uint64_t build_shadow_samples;  /* shadow-march iterations of the last build */
  uint64_t bytes;                 /* of the lattice */
  double build_ms;                /* device time of the last build */
} ovr_hip_shadow_cache;
int ovr_hip_get_shadow_cache(const ovr_hip_renderer* r, ovr_hip_shadow_cache* out);
/* the lattice of `member` (0 for a single renderer) as the next cached frame would read it - mode CACHED builds it first if it is stale (needs a volume and a
 * transfer function) - and its nodes' world positions (3 floats per node; may be NULL, like values_host).  dims is always filled; the arrays only when
 * capacity_nodes holds the lattice (EINVAL otherwise).  ESTATE in mode MARCHED. */
int ovr_hip_get_shadow_cache_values(ovr_hip_renderer* r, int32_t member, int32_t dims[3], float* values_host, float* positions_host, size_t capacity_nodes);

/* replaces DeviceOptix7::Impl::commit (device_impl.cpp:113-197): applies every queued setter; any change resets
 * the accumulation (frame_index restarts at 1 on the next render). */
int ovr_hip_commit(ovr_hip_renderer* r);

/* replaces DeviceOptix7::render (optix7/device.cpp:35-43, device_impl.cpp:199-269): one frame, blocking until the
 * frame is complete on the device; adds the elapsed milliseconds to the value ovr_hip_render_time_ms() returns. */
int ovr_hip_render(ovr_hip_renderer* r);
/* non-blocking variant: enqueues the frame on the renderer's stream and returns (hipEvent timing around it, overlap with the caller's other work -
 * e.g. the gather of the previous frame).  The first frame after a camera / volume / size / spp / jitter change reads 8 bytes back from the device
 * before it launches - how many 8x8-pixel blocks have a ray that meets the volume's box; the others get no workgroup, their pixels are cleared - a
 * stream synchronisation of ~20 us (a device group's members wait side by side, each on its own host thread).  A frame is NOT a unit for hipGraph
 * capture - it records timed events and its counters are read by the host when it is resolved: with a caller's stream (ovr_hip_set_stream) that is
 * capturing, the call fails with OVR_HIP_ESTATE and leaves the capture intact.  (A frame is five launches, ~10 us of host time that overlap its
 * first kernel: there is nothing for a graph to take) */
int ovr_hip_render_async(ovr_hip_renderer* r);
/* waits for the frame enqueued by render_async and for everything else enqueued on the renderer's stream
 * (ovr_hip_pack_tiles / ovr_hip_unpack_tiles launches included) */
int ovr_hip_sync(ovr_hip_renderer* r);

/* replaces Impl::mapframe (device_impl.cpp:271-281): publishes the CURRENT framebuffer set.
 * mem_kind DEVICE: device pointers (as the reference hands out, CrossDeviceBuffer::DEVICE_CUDA);
 * mem_kind HOST: the frame is copied to pinned host memory owned by the renderer (what the caller's
 * CrossDeviceBuffer::to_cpu() would do, cross_device_buffer.h:130-159) and stays valid until the next mapframe
 * of the same set.  rgba = W*H*4 floats, row 0 = bottom; grad = W*H*3 floats (may be NULL to skip). */
int ovr_hip_mapframe(ovr_hip_renderer* r, int mem_kind, const float** rgba, size_t* rgba_bytes, const float** grad,
                     size_t* grad_bytes);
/* frame output: image_to_rgba8 of the reference (ovr/common/imageio.cpp:146-181: clamp to [0,1], * 255,
 * truncate; `flip_vertical` as renderbatch passes it, apps/main_batch.cpp save_image) applied to the CURRENT framebuffer
 * set on the device - the host copy of a saved or displayed frame is 4 bytes per pixel instead of 16.  The pointer
 * stays valid until the next call of this function or a framebuffer resize. */
int ovr_hip_mapframe_rgba8(ovr_hip_renderer* r, int mem_kind, int flip_vertical, const uint32_t** rgba8, size_t* bytes);

/* frame output, EXR: the float -> half step of the reference's save_image(".exr") (ovr/common/imageio.cpp:15-83,
 * 268-272: the flipped RGBA32F frame goes to tinyexr with requested_pixel_types = HALF; conversion rule
 * extern/tinyexr/tinyexr.h:889-924 - nearest, ties away from zero) applied to the CURRENT framebuffer set on the device:
 * W*H*4 IEEE binary16 bit patterns (R, G, B, A per pixel).  Valid until the next call or a framebuffer resize. */
int ovr_hip_mapframe_rgba16f(ovr_hip_renderer* r, int mem_kind, int flip_vertical, const uint16_t** rgba16f, size_t* bytes);

/* replaces Impl::swap (device_impl.cpp:102-111): waits for the current set's stream, flips to the other set */
int ovr_hip_swap(ovr_hip_renderer* r);

/* MainRenderer::render_time (ovr/renderer.h:87): accumulated milliseconds spent in ovr_hip_render */
double ovr_hip_render_time_ms(const ovr_hip_renderer* r);
int ovr_hip_get_stats(const ovr_hip_renderer* r, ovr_hip_stats* out);

/* what load_from_array3d_scalar leaves behind (volume.cpp:181-191): the data range found by compute_scalar_range /
 * cuda_scalar_range (array.cpp:27-66,92-108,297; integer-normalized for 8- and 32-bit integer volumes, raw otherwise), the
 * transfer-function range in effect (set_value_range, volume.cpp:131-145: a range with hi < lo keeps the previous one, which is
 * the data range after a load) and the bytes the re-laid-out volume occupies in HBM */
typedef struct ovr_hip_volume_info {
  int32_t dims[3];
  int32_t value_type;      /* OVR_HIP_TYPE_* as passed to ovr_hip_set_volume */
  uint64_t resident_bytes;
  float data_lower, data_upper;
  float tf_lower, tf_upper;
} ovr_hip_volume_info;
int ovr_hip_get_volume_info(const ovr_hip_renderer* r, ovr_hip_volume_info* out);

/* multi-GPU helpers.  pack: copies this rank's tiles out of its W*H framebuffer into a compact
 * [n_owned_tiles][tile_h][tile_w][4] device buffer (the RCCL gather payload); unpack: scatters the gathered payload
 * of `src_rank` into a W*H*4 frame on the gathering rank.  Both run on the renderer's stream. */
int ovr_hip_owned_tiles(const ovr_hip_renderer* r, int32_t rank, int32_t* n_tiles);
int ovr_hip_pack_tiles(ovr_hip_renderer* r, float* dst_device, size_t dst_bytes);
int ovr_hip_unpack_tiles(ovr_hip_renderer* r, int32_t src_rank, const float* src_device, size_t src_bytes,
                         float* frame_device, size_t frame_bytes);
/* all ranks' payloads in one launch: rank k's payload starts at src_device + k * rank_stride_bytes (the receive
 * buffer of the gather as one allocation); rank_stride_bytes is a multiple of 16 and >= the largest payload */
int ovr_hip_unpack_all_tiles(ovr_hip_renderer* r, const float* src_device, size_t rank_stride_bytes, size_t src_bytes,
                             float* frame_device, size_t frame_bytes);

/* stand-alone pieces of the path, exposed for known-answer tests through the same ABI (device buffers) */
/* ovr/common/generate_mask.cu:100-120: compacted (x,y) list for this frame; returns the int32 count in *n_out */
int ovr_hip_sparse_mask(ovr_hip_renderer* r, int32_t frame_index, int32_t* out_xy_device, size_t out_bytes,
                        int64_t* n_out);
/* ovr/common/random/random.h:146-188: n (v0,v1) states -> 2n floats, states advanced in place */
int ovr_hip_tea_floats(ovr_hip_renderer* r, uint32_t* v0v1_device, float* out_device, int64_t n);

/* ABI v10 - shaders_raymarching.cu:64-66,118-122: the `__powf(x, y)` of the opacity correction as the kernels evaluate it, n (x, y) pairs -> n floats
 * (device buffers).  which = 0: the pow this library was built with - v_exp_f32(y * v_log_f32(x)), CUDA's documented structure of the intrinsic, in
 * the product; 1: a machine-independent log2 / exp2 pair (fmaf Horner chains; the CPU oracle's mode 2 is the same arithmetic, bit for bit).  A library
 * built with -DOVR_PARITY_EXACT=1 (libovr_hip_parity.so: a test instrument for the parity tests, never the product - ovr_hip_built_for_exact_parity() == 1)
 * marches with that pair: every sample count then equals the oracle's exactly, which pins the transcendental's last bit as the one source of the
 * tolerated count differences. */
int ovr_hip_pow_floats(ovr_hip_renderer* r, const float* x_device, const float* y_device, float* out_device, int64_t n, int32_t which);
int ovr_hip_built_for_exact_parity(void);
/* the shade factor as the kernels evaluate it (added with the light and material entry points): n (world normal, world position, shadow) triples -> n floats (device buffers; normal_w and
 * pos hold 3 floats per sample), through the device function the frame's shading calls, with the committed light, material and camera position. */
int ovr_hip_shade_floats(ovr_hip_renderer* r, const float* normal_w_device, const float* pos_device, const float* shadow_device, float* out_device, int64_t n);
/* the box test as the kernels evaluate it (added with the clip box): n world-space rays (3 floats each for origin and direction; the direction is used as given)
 * -> n triples (t0, t1, hit ? 1 : 0) (device buffers), through the device function the march, the shadow march and the schedule call, with the committed
 * volume transform and clip box - without a clip box the unit cube's result.  Needs a volume. */
int ovr_hip_clip_intervals(ovr_hip_renderer* r, const float* org_device, const float* dir_device, float* t0t1hit_device, int64_t n);
/* the shadow term as the kernels evaluate it (added with the shadow cache): n world positions (3 floats each) -> n floats (device buffers).  which = 0: the
 * shadow march, through the device function the marched frame's shading calls, with the committed light, sampling rate, transfer function and clip box (works
 * in every mode; needs a volume and a transfer function); which = 1: the lattice lookup of the cached frame's shading (ESTATE in mode MARCHED; mode CACHED
 * builds a stale lattice first). */
int ovr_hip_shadow_floats(ovr_hip_renderer* r, const float* pos_device, float* out_device, int64_t n, int32_t which);
/* a projection as the kernels evaluate it (added with the projections): n world-space rays (3 floats each for origin and direction; the direction is used as
 * given) -> 4 floats each (device buffers): v, tm*, steps, fetched steps - four zeros for a ray that is not marched -, four lanes per ray through the device
 * function the projection frame's kernel calls, with the committed volume transform, sampling rate and clip box.  mode (1 ... 3) and range_skipping come from
 * the arguments: it works while the committed mode is OFF, and before a transfer function is committed (none is read; the addressing rule then counts the
 * tables as empty, which can pick another addressing mode than a frame's - every mode gives the same values).  ESTATE without a volume; EINVAL: a null
 * pointer, n < 0, mode not in 1 ... 3. */
int ovr_hip_project_floats(ovr_hip_renderer* r, const float* org_device, const float* dir_device, float* out_device, int64_t n, int32_t mode, int32_t range_skipping);
/* an isosurface ray as the kernels evaluate it (added with the isosurfaces): n world-space rays as for ovr_hip_project_floats -> 8 floats each (device buffers):
 * hit (0 / 1), isovalue, t*, steps walked, the world normal (x, y, z), the shadow term - through the device function the isosurface frame's kernel calls under full
 * shading (normal and shadow are always computed), with the COMMITTED isovalues, volume transform, sampling rate, light and clip box; a ray without a hit gives zeros
 * but for the steps walked.  range_skipping comes from the argument.  ESTATE without a volume or while no isovalue is committed; EINVAL: a null pointer, n < 0. */
int ovr_hip_isosurface_floats(ovr_hip_renderer* r, const float* org_device, const float* dir_device, float* out_device, int64_t n, int32_t range_skipping);
/* a translucent isosurface ray as the kernels evaluate it (added with the translucent isosurfaces): four lanes per ray through the device function the translucent
 * frame's kernel calls, under full shading, with the COMMITTED isovalues, opacities, light, sampling rate and clip box (all-ones opacities included).  max_events
 * in 1 ... 16.  Per ray 4 + 8 * max_events floats: (events composited, A, steps walked, shadow steps over all events), then per event e < min(events, max_events)
 * (k, t*, n_w.x, n_w.y, n_w.z, shadow, A after the event, 0); the rest zeros.  ESTATE without a volume or isovalues; EINVAL: a null pointer, n < 0, a bad max_events. */
int ovr_hip_isosurface_layers_floats(ovr_hip_renderer* r, const float* org_device, const float* dir_device, float* out_device, int64_t n, int32_t max_events, int32_t range_skipping);
/* an isosurface ray with ambient occlusion as the kernels evaluate it (added with the ambient occlusion): four lanes per ray through the device function the AO
 * frame's kernel calls, under full shading, with the COMMITTED isovalues, opacities, AO samples and distance, light, sampling rate and clip box, every ray at the
 * rotation `rotation` (0 ... 15) of the direction table.  max_events in 1 ... 16.  Per ray 8 + 8 * max_events floats: the layers entry's header (events composited,
 * A, steps walked, shadow steps over all events) followed by (the AO walks' steps walked, the AO walks' fetched steps, 0, 0), then per event
 * e < min(events, max_events) the layers entry's record with O in its last slot: (k, t*, n_w.x, n_w.y, n_w.z, shadow, A after the event, O); the rest zeros.
 * ESTATE without a volume, isovalues or committed AO samples; EINVAL: a null pointer, n < 0, a bad max_events or rotation. */
int ovr_hip_isosurface_ao_floats(ovr_hip_renderer* r, const float* org_device, const float* dir_device, float* out_device, int64_t n, int32_t max_events, int32_t rotation,
                                 int32_t range_skipping);
/* a slice ray as the kernels evaluate it (added with the slices): n world-space rays as for ovr_hip_project_floats - the direction used as given - through the
 * device function the slice frame's kernel calls, with the COMMITTED slices, volume transform, sampling rate and clip box.  Per ray 4 floats: (the winning
 * slice's index + 1 or 0, v, t_k, steps walked - 1 for a plane); zeros for a ray that meets nothing.  ESTATE without a volume or without committed slices;
 * EINVAL: a null pointer, n < 0. */
int ovr_hip_slice_floats(ovr_hip_renderer* r, const float* org_device, const float* dir_device, float* out_device, int64_t n, int32_t range_skipping);
/* a context ray as the kernel evaluates it (added with the slice context): n world-space rays as for ovr_hip_slice_floats through the device function the context
 * frame's kernel calls, with the COMMITTED slices, opacity scale, transfer function, volume transform, sampling rate and clip box.  Per ray 8 floats: (the
 * composited slice's index + 1 or 0, v, t_k, context steps taken, r, g, b, a of the pixel sample).  ESTATE without a volume, without committed slices or while the
 * committed context mode is OFF; EINVAL: a null pointer, n < 0. */
int ovr_hip_slice_context_floats(ovr_hip_renderer* r, const float* org_device, const float* dir_device, float* out_device, int64_t n);
/* an isosurface context ray as the kernel evaluates it (added with the isosurface context): n world-space rays as for ovr_hip_isosurface_layers_floats, four
 * lanes each, through the device function the context frame's kernel calls, under full shading, with the COMMITTED isovalues, opacities, opacity scale, transfer
 * function, light, material, volume transform, sampling rate and clip box.  Per ray 8 + 8 * max_events floats (max_events in 1 ... 16): (events composited, A, steps
 * walked, shadow steps, r, g, b of the pixel sample, volume samples with a' > 0), then ovr_hip_isosurface_layers_floats' record per event (k, t*, the world normal,
 * the shadow term, A after the event, 0).  ESTATE without a volume, a transfer function or isovalues, or while the committed context mode is OFF; EINVAL: a null
 * pointer, n < 0, max_events outside 1 ... 16. */
int ovr_hip_isosurface_context_floats(ovr_hip_renderer* r, const float* org_device, const float* dir_device, float* out_device, int64_t n, int32_t max_events);
/* a pre-integrated ray as the kernel evaluates it (added with pre-integrated classification): n world-space rays as for ovr_hip_slice_floats through the device
 * function the pre-integrated frame's kernel calls, with the COMMITTED transfer function, volume transform, sampling rate and clip box - whatever frame kind and
 * shading mode are committed.  Per ray 8 floats: segments taken, of them integral-branch segments, tx at exit, 0, r, g, b, a of the pixel sample.  ESTATE without a
 * volume, while the committed mode is OFF or without a committed transfer function; EINVAL: a null pointer, n < 0. */
int ovr_hip_preintegrated_floats(ovr_hip_renderer* r, const float* org_device, const float* dir_device, float* out_device, int64_t n);
/* a gradient-opacity ray as the kernel evaluates it (added with gradient opacity): n world-space rays as for ovr_hip_slice_floats through the device function
 * the gradient-opacity frame's kernel calls, with the COMMITTED thresholds, transfer function, volume transform, sampling rate, clip box, light and material -
 * whatever frame kind and shading mode are committed - under shading `shade`: 0 (NONE) or 1 (GRADIENT; the view vector is the perspective camera's).  Per ray 8
 * floats: steps taken, of them steps that fetched a gradient, tx at exit, steps with a > 0, r, g, b, a of the pixel sample.  ESTATE without a volume, while the
 * committed mode is OFF or without a committed transfer function; EINVAL: a null pointer, n < 0, shade outside {0, 1}. */
int ovr_hip_gradient_opacity_floats(ovr_hip_renderer* r, const float* org_device, const float* dir_device, float* out_device, int64_t n, int32_t shade);
/* a depth-limited ray as the kernel evaluates it (added with the depth limit): n world-space rays as for ovr_hip_slice_floats, ray i ending on depth_device[i]
 * (the march's t, as for ovr_hip_set_max_depth), through the device function the depth-limited frame's kernel calls, with the COMMITTED transfer function,
 * volume transform, sampling rate, clip box, light and material - whatever frame kind, shading mode and depth image are committed - under shading `shade`: 0
 * (NONE) or 1 (GRADIENT; the view vector is the perspective camera's).  Per ray 8 floats: steps taken, the cut tc, tx at exit, steps with a > 0, r, g, b, a of
 * the pixel sample (tc and tx 0 for a ray that misses the box).  ESTATE without a volume or without a committed transfer function; EINVAL: a null pointer,
 * n < 0, shade outside {0, 1}. */
int ovr_hip_max_depth_floats(ovr_hip_renderer* r, const float* org_device, const float* dir_device, const float* depth_device, float* out_device, int64_t n, int32_t shade);
/* a depth-output ray as the kernel evaluates it (added with the depth layer): as ovr_hip_max_depth_floats, through the device function the depth frame's kernel
 * calls, with crossing threshold `threshold`; depth_device == NULL means no limit on any ray.  Per ray 12 floats: the depth limit's eight, then reached (0 / 1),
 * d, k, S.  Needs nothing committed but volume and transfer function (ESTATE without).  EINVAL: a null org, dir or out, n < 0, shade outside {0, 1}, a
 * threshold ovr_hip_set_depth_output refuses. */
int ovr_hip_depth_output_floats(ovr_hip_renderer* r, const float* org_device, const float* dir_device, const float* depth_device_or_null, float* out_device, int64_t n, int32_t shade, float threshold);
/* the pixel rays as the kernels form them (added with the orthographic camera): the world origin and direction of sample `sample` (0 ... spp - 1) of frame
 * `frame_index` (1-based) for every pixel, width x height x 6 floats in image order (a device buffer of capacity_floats floats) - through the device function
 * every frame kernel calls, with the COMMITTED camera, framebuffer size, jitter mode, noise tile and samples per pixel.  Needs a committed framebuffer and no
 * volume.  EINVAL: a null pointer, frame_index < 1, a sample outside 0 ... spp - 1, a capacity below width x height x 6; ESTATE: no framebuffer size. */
int ovr_hip_camera_rays(ovr_hip_renderer* r, int32_t frame_index, int32_t sample, float* org_dir_device, size_t capacity_floats);

#ifdef __cplusplus
}
#endif
#endif /* OVR_HIP_H */
