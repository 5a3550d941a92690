// state.hpp - what the host units share: the error channel, the queued parameter values, the renderer's state and the functions one unit
// offers the others.  buffers.cpp / volume.cpp / frame.cpp / group.cpp each own one part of the state machine; ../ovr_hip_api.cpp is the
// extern "C" layer over them.  Everything declared here is internal to libovr_hip.so (hidden visibility): the library exports
// include/ovr_hip.h and nothing else.
#pragma once

#include "../../../include/ovr_hip.h"
#include "../ovr_hip_kernels.h"
#include "../ovr_hip_update.h"
#pragma GCC visibility push(hidden)
#include "commit_plan.hpp"
#include "depth_output_host.hpp"
#include "gradient_opacity_host.hpp"
#include "max_depth_host.hpp"
#include "policy.hpp"
#include "slices_host.hpp"
#pragma GCC visibility pop

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

struct ovr_hip_renderer;
struct GroupWorker; // one host thread per follower of a device group (group.cpp)

namespace ovrhip {
namespace host __attribute__((visibility("hidden"))) {

inline thread_local std::string g_last_error;

inline int fail(int code, const std::string& msg)
{
  g_last_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                                                  \
  do {                                                                                                                 \
    hipError_t e__ = (expr);                                                                                           \
    if (e__ != hipSuccess)                                                                                             \
      return fail(OVR_HIP_EDEVICE, std::string("[hip] ") + #expr + " failed: " + hipGetErrorString(e__));            \
  } while (0)

struct V3 { float x, y, z; };
inline V3 sub(V3 a, V3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline float dot(V3 a, V3 b) { return std::fmaf(a.x, b.x, std::fmaf(a.y, b.y, a.z * b.z)); }
inline V3 cross(V3 a, V3 b) { return { a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y }; }
inline V3 normalize(V3 v) { const float l = std::sqrt(dot(v, v)); return { (v.x * 1.f) / l, (v.y * 1.f) / l, (v.z * 1.f) / l }; }
inline V3 scale(float s, V3 a) { return { s * a.x, s * a.y, s * a.z }; }

template <typename T> struct Queued { // vidi::TransactionalValue (ovr/common/vidi_transactional_value.h:26-168), minus the template
  T queued{}, current{};
  bool dirty = false;
  void init(const T& v) { queued = current = v; } // a default: committed without a commit
  void set(const T& v) { queued = v; dirty = true; }
  bool update() { if (!dirty) return false; current = queued; dirty = false; return true; }
};

// kind: OVR_HIP_CAMERA_*; fovy belongs to the perspective, height (the image's world height) to the orthographic camera
struct CameraP { float from[3] = { 0, 0, 0 }, at[3] = { 0, 0, -1 }, up[3] = { 0, 1, 0 }; float fovy = 60.f; int kind = OVR_HIP_CAMERA_PERSPECTIVE; float height = 0.f; };
struct FocusP { float cx = 0.5f, cy = 0.5f, scale = 0.2f, base_noise = 0.1f; }; // params.h:82-84
struct TfnP { std::vector<float> colors, alphas; float lo = 1, hi = -1; };
struct ShardP { int rank = 0, world = 1, tw = 64, th = 64; };
struct Size2 { int w = 0, h = 0; };
struct ConvP { int mode = OVR_HIP_CONVERGENCE_OFF; float threshold = 0.f; };
// a: the isovalues' opacities in (0, 1], travelling with v (ovr_hip_set_isosurface_layers); 1 behind n and after ovr_hip_set_isosurfaces
struct IsoP {
  int n = 0;
  float v[OVR_HIP_MAX_ISOVALUES] = { 0.f, 0.f, 0.f, 0.f };
  float a[OVR_HIP_MAX_ISOVALUES] = { 1.f, 1.f, 1.f, 1.f };
  bool translucent() const { for (int k = 0; k < n; ++k) if (a[k] < 1.f) return true; return false; }
};
// ovr_hip_set_slices, as the host derives them (slice_values in slices_host.hpp): the unit normal, c = dot(n, point), the thickness as given and the mode (kept
// as given; read only while thickness > 0); the entries behind n are zeros
struct SliceP {
  int n = 0;
  float normal[OVR_HIP_MAX_SLICES][3] = {};
  float c[OVR_HIP_MAX_SLICES] = {}, thickness[OVR_HIP_MAX_SLICES] = {};
  int mode[OVR_HIP_MAX_SLICES] = {};
  bool walks() const { for (int k = 0; k < n; ++k) if (thickness[k] > 0.f) return true; return false; }
};
// ovr_hip_set_slice_context: the mode (OVR_HIP_SLICE_CONTEXT_*) and the opacity scale in [0, 1], stored as 1 in mode OFF
struct SliceContextP { int mode = 0; float scale = 1.f; };
// ovr_hip_set_isosurface_context: the mode (OVR_HIP_ISO_CONTEXT_*) and the opacity scale in [0, 1], stored as 1 in mode OFF
struct IsoContextP { int mode = 0; float scale = 1.f; };
// ovr_hip_set_preintegration: the mode (OVR_HIP_PREINTEGRATION_*)
struct PreintP { int mode = 0; };
// ovr_hip_set_ambient_occlusion: K and the radius (+inf while K == 0: the radius is not read then)
struct AoP { int samples = 0; float distance = INFINITY; };
// ovr_hip_set_light / ovr_hip_set_material.  The defaults are the reference's literals: its light vector (params.h:79), light_rgb = 2 = intensity 1
// and the 0.5 / 0.5 of its shade expression (shaders_raymarching.cu:138,156-157)
struct LightP { float dir[3] = { -907.108f, 2205.875f, -400.0267f }; float intensity = 1.f; };
struct MaterialP { float ambient = 0.5f, diffuse = 0.5f, specular = 0.f, shininess = 0.f; };
// ovr_hip_set_clip_box: the world box as given (-inf / +inf: open on that side).  The object box the kernels test is derived from it and the volume
// (apply_clip_box)
struct ClipP { int enabled = 0; float lower[3] = { -INFINITY, -INFINITY, -INFINITY }, upper[3] = { INFINITY, INFINITY, INFINITY }; };
// ovr_hip_set_shadow_cache: the mode and the cell size in voxels (0 resolved to the default by the setter)
struct ShadowP { int mode = OVR_HIP_SHADOWS_MARCHED; int cell = ovrhip::policy::kShadowCacheDefaultCell; };

// ---- shadow cache (ovr_hip_set_shadow_cache).  No buffer exists until a mode other than MARCHED needs one.
struct ShadowCacheState {
  float* d_built = nullptr;          // mode CACHED: the lattice of the shadow march's values
  size_t built_cap = 0;              // nodes d_built holds
  int built_dims[3] = { 0, 0, 0 };
  bool built_valid = false;          // d_built is current (commit::kLatticeStale clears it)
  float* d_supplied = nullptr;       // mode SUPPLIED: the caller's lattice (ovr_hip_set_shadow_cache_values)
  int supplied_dims[3] = { 0, 0, 0 };
  unsigned long long* d_iterations = nullptr; // the build's iteration counter
  hipEvent_t ev[2] = { nullptr, nullptr };
  uint64_t builds = 0, build_samples = 0;
  double build_ms = 0.0;
};

// the frame words on the device (ovr_hip_renderer::d_counters): 8 counters, the pool's control words from byte 128, the reduction's ticket word behind them
constexpr size_t kFrameWordsBytes = 128 + (size_t)ovrhip::kPoolCtrlWords * sizeof(unsigned int) + 128;
constexpr size_t kReconWords = 2 + 64; // ReconParams::words

// ---- convergence estimate and adaptive refinement (ovr_hip_set_convergence).  The buffers exist only while the mode is not OFF.
struct ConvergenceState {
  float* d_accum_half = nullptr;        // H: the sum of the even-numbered frames (W*H*4)
  float* d_grad_keep = nullptr;         // adaptive: the gradient pixels of the retired blocks (W*H*3)
  float* d_error = nullptr;             // per block of the image (bx + by * ceil(W / 8)): E_b
  int* d_frames = nullptr;              // per block: the even frame of its estimate, negated when retired, 0 = none
  unsigned int* d_words = nullptr;      // ConvergenceParams::words
  unsigned int* d_lists = nullptr;      // adaptive: [active: list_cap][retired: list_cap][counts]
  unsigned int* h_publish = nullptr;    // pinned: ConvergenceParams::publish
  size_t blocks = 0, list_cap = 0;
  const unsigned int* sorted = nullptr; // the frame's launch list before anything was retired from it
  bool frame = false;                   // the frame in flight is followed by an estimate
  bool resolve_only = false;            // the frame in flight marches nothing: every block is retired
  bool valid = false;
  float error = 0.f;
  int frames = 0;
  unsigned int active = 0, retired = 0; // entries of the launch list that are marched / resolved (active + retired == sched.n_work while adaptive)
};

// ---- pull-push reconstruction of sparse-sampled frames (ovr_hip_set_reconstruction).  The buffers exist only while the mode is FILL.
struct ReconstructionState {
  float* d_count = nullptr;          // N: per pixel, the frames that sampled it (W*H)
  float* d_grad = nullptr;           // G: the gradient layer of the sampled pixels, accumulated like A (W*H*3)
  float4* d_pyramid = nullptr;       // levels >= 1, two float4 per texel
  unsigned int* d_words = nullptr;   // ReconParams::words (kReconWords)
  unsigned int* h_publish = nullptr; // pinned: ReconParams::publish
  hipEvent_t ev[2] = { nullptr, nullptr };
  bool frame = false;                // the frame in flight is reconstructed behind its last kernel
  bool timed = false;                // ... between ev[0] and ev[1]
  bool accumulated = false;          // the last reconstructed frame accumulated: G is defined
  ReconParams params{};
  ovr_hip_reconstruction info{};
};

// launch order of the march's 8x8-pixel workgroups (dense mode): owned blocks, longest rays first
struct ScheduleState {
  unsigned int* d_src = nullptr;    // owned blocks in image order (host-built: framebuffer size and shard)
  unsigned int* d_sorted = nullptr; // sorted on the device whenever the camera or the volume's box changes
  unsigned int n = 0;
  bool list_dirty = true, dirty = true;
  // Blocks none of whose rays meets the volume's box are not launched (round 4; launch_schedule's `exact` classification puts them last in the
  // list): n_work = the entries that get a march / composite workgroup, empty_pixels = the active pixels of the others (they count as rays and
  // rendered pixels like before).  Their pixels are zeroed by launch_clear_blocks - once per framebuffer set after anything changed (clear_gen),
  // and on the first frame of an accumulation (the accumulation buffer's turn).
  unsigned int* h_info = nullptr;   // pinned: the scatter kernel writes { n_work, empty_pixels } into it
  unsigned int n_work = 0, empty_pixels = 0, frame_empty_pixels = 0;
  unsigned long long frame_empty_rays = 0;
  unsigned int clear_gen = 1, set_clear_gen[2] = { 0, 0 };
  int exact = 0;
};

// ---- device group (ovr_hip_create_group): one process drives several GPUs, each member renders the image tiles of rank `rank` of
// members.size() (ovr_hip_set_image_shard semantics, volume replicated) and the leader - members[0], the handle the caller holds - gathers the
// followers' tiles into its own framebuffer at the end of every frame.  A follower is an ordinary renderer whose `leader` is set.
struct GroupState {
  std::vector<ovr_hip_renderer*> members; // leader only: every member, itself first
  // A setter on a group queues its value on every member; ovr_hip_commit applies the queued values member by member.  Both hold this mutex of the
  // leader, so a commit on the render thread never falls between the members of one setter call on the GUI thread (a frame whose tiles come from
  // two cameras); the reference's TransactionalValue gives the same guarantee per value (vidi_transactional_value.h:75-103)
  std::mutex mtx;
  ovr_hip_renderer* leader = nullptr;     // follower only
  int rank = 0;
  int gather_kind = 0;                    // leader: 0 = no group, 1 = peer copies, 2 = RCCL send / recv
  hipStream_t comm_stream = nullptr;      // every member: where its payload travels (the render stream goes on with the next frame)
  hipEvent_t ev_packed = nullptr, ev_shipped = nullptr; // on the member's own device: its tiles are packed / have left on its comm_stream (peer copies)
  hipEvent_t ev_received = nullptr;       // follower, created on the LEADER's device: its tiles have arrived on the leader's comm_stream (RCCL) - an
                                          // event is recorded on a stream of its own device only
  bool shipped_by_rccl = false;           // which of the two events the leader's scatter waits for
  float* d_payload[2] = { nullptr, nullptr };  // follower: its packed tiles, [0] RGBA, [1] gradient layer
  float* d_gather[2] = { nullptr, nullptr };   // leader: every member's payload, stride[] floats apart
  size_t payload_floats[2] = { 0, 0 }, stride[2] = { 0, 0 };
  int fb[5] = { 0, 0, 0, 0, 0 };          // what the gather buffers were sized for: W, H, tile_w, tile_h, size
  bool grad = true;                       // the gradient layer travels too (OVR_HIP_MAP_GRAD=0: RGBA only, like the plugin's mapframe)
  void* rccl_comm = nullptr;              // every member of an RCCL group: its communicator
  ovr_hip_stats own_stats{};              // leader: its own frame's counters (ovr_hip_renderer::stats holds the group's sums)
  double gather_ms = 0.0;                 // leader: host time of the last frame's gather tail (after the slowest member's frame: wait for the shipments + scatter)
  double upload_ms = 0.0;                 // leader: wall time of the last volume upload over all members
  double update_ms = 0.0;                 // leader: ... of the last ovr_hip_update_volume
  // Round 5: every follower has a host thread of its own (device set once, persistent): the leader posts commit / render_async / ship / finish to all of
  // them and waits on their counters, so the members' frames are enqueued side by side instead of one after the other (one thread driving 8 members
  // spent 225 us per frame on it, beside 485 us of device time per member).
  GroupWorker* worker = nullptr;          // follower only
  hipEvent_t ev_gathered = nullptr;       // leader, RCCL: behind the ONE grouped receive of a frame on its comm_stream
  // A member whose commit or volume upload failed leaves the group in mixed state: the group refuses to render until a commit has
  // succeeded on every member AND they agree on what was committed / until a volume upload has succeeded on all of them
  bool broken = false;
  std::string broken_why;
  double host_us[4] = { 0, 0, 0, 0 };     // leader: host time of the last frame's steps (enqueue, ship, finish, scatter), microseconds
};

} // namespace host
} // namespace ovrhip

struct ovr_hip_renderer {
  template <typename T> using Queued = ovrhip::host::Queued<T>;
  int device = 0;
  std::mutex mtx; // protects the queued values (setters may come from any thread)
  hipStream_t own_stream[2] = { nullptr, nullptr };
  hipStream_t user_stream = nullptr;
  bool use_user_stream = false;
  hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };

  // queued values (setters), applied by ovr_hip_commit
  Queued<ovrhip::host::Size2> fbsize;
  Queued<ovrhip::host::CameraP> camera;
  Queued<ovrhip::host::TfnP> tfn;
  Queued<ovrhip::host::FocusP> focus;
  Queued<int> spp, sparse, accumulate, shading, grid_convention, pipeline, skipping, jitter, lds_staging;
  Queued<int> projection;   // ovr_hip_set_projection: OVR_HIP_PROJECT_*; recorded under the commit plan's source kShading
  bool projection_skipped = false; // the last projection frame ran the range-skipping kernel (ovr_hip_get_projection)
  Queued<ovrhip::host::IsoP> isosurfaces; // ovr_hip_set_isosurfaces: sorted ascending; recorded under kShading like the projection mode.  n > 0: isosurface frames
  bool isosurface_skipped = false; // the last isosurface frame ran the range-skipping kernel (ovr_hip_get_isosurfaces)
  Queued<ovrhip::host::AoP> ambient_occlusion; // ovr_hip_set_ambient_occlusion; recorded under kShading like the isovalues
  Queued<ovrhip::host::SliceP> slices; // ovr_hip_set_slices; recorded under kShading like the projection mode.  n > 0: slice frames, whatever isovalues and projection mode are committed
  bool slices_skipped = false;     // the last slice frame ran the range-skipping kernel (ovr_hip_get_slices)
  Queued<ovrhip::host::SliceContextP> slice_context; // ovr_hip_set_slice_context; recorded under kShading like the slices.  Kept while no slice is committed: it takes effect when n > 0
  Queued<ovrhip::host::IsoContextP> isosurface_context; // ovr_hip_set_isosurface_context; recorded under kShading like the isovalues.  Kept while no isovalue is committed: it takes effect when n > 0 and no slice is committed
  Queued<ovrhip::GradientOpacityState> gradient_opacity; // ovr_hip_set_gradient_opacity (host/gradient_opacity_host.hpp); recorded under kShading like the other frame kinds.  Kept, and not drawn, while gradient_opacity_frame says no
  // ovr_hip_set_max_depth (host/max_depth_host.hpp); recorded under kShading like the other frame kinds: every call with an image counts as a change.  Kept, and
  // not drawn, while max_depth_frame says no.  The images: the setter copies into d_max_depth_queued (it only ever grows), a commit that applies an image swaps the
  // two buffers; d_max_depth holds max_depth.current.width x height floats while max_depth.current.on
  Queued<ovrhip::MaxDepthState> max_depth;
  float* d_max_depth = nullptr;
  float* d_max_depth_queued = nullptr;
  size_t max_depth_capacity = 0, max_depth_queued_capacity = 0; // floats the two buffers hold
  Queued<ovrhip::DepthOutputState> depth_output; // ovr_hip_set_depth_output (host/depth_output_host.hpp); recorded under kShading like the other frame kinds.  Kept, and not drawn, while depth_output_frame says no
  Queued<ovrhip::host::PreintP> preintegration; // ovr_hip_set_preintegration; recorded under kShading like the other frame kinds.  Kept, and not drawn, while the committed frame is not the unshaded march
  // the integral node table of the committed transfer function (host/preintegration_host.hpp): built by the first pre-integrated frame (or tables getter) after a
  // transfer-function commit - it carries the generation of the tables it was built from and the subdivision the frame's LDS budget allowed
  std::vector<float> preint_table; // 4 * (M + 1) floats, as uploaded to d_preint_nodes
  float* d_preint_nodes = nullptr;
  size_t preint_capacity = 0;      // floats d_preint_nodes holds
  int preint_nodes = 0, preint_subdivision = 0; // M and S of the table; 0: none yet
  unsigned long long preint_generation = 0;     // tf_generation of the tables it was built from
  std::vector<float> ao_table;     // the direction table of the committed K, [16][K][3], as uploaded to d_ao_dirs (both follow K at commit)
  float* d_ao_dirs = nullptr;
  Queued<float> rate;
  Queued<ovrhip::host::ShardP> shard;
  Queued<ovrhip::host::LightP> light;        // the raw vector: normalised when it is applied (unit_light)
  Queued<ovrhip::host::MaterialP> material;
  Queued<ovrhip::host::ClipP> clip;          // the world box: the object box follows the volume (apply_clip_box)
  Queued<ovrhip::host::ShadowP> shadow;      // the shadow cache's mode and cell size
  Queued<ovrhip::host::ConvP> convergence;
  Queued<int> reconstruction;
  Queued<int> layouts;      // ovr_hip_set_volume_layouts: which replicas the next ovr_hip_set_volume plans (2: builds at once)
  Queued<int> layout_choice; // -1 = automatic (camera direction / the previous frame's work), 0..3 = forced (falls back to general if not resident)

  // volume: d_volume / vd = the general layout (always resident); replica[1..2] = the thin layouts, [3] = the quad layout (ovr_hip_kernels.h), if built
  void* d_volume = nullptr;
  std::atomic<size_t> volume_bytes{ 0 }; // all resident replicas (a builder thread adds its replica's)
  ovrhip::VolumeDesc vd{};
  void* d_replica[ovrhip::kLayouts] = {};  // [3] = the quad replica (f32 volumes)
  void* d_axis[ovrhip::kLayouts] = {}; // per layout: its per-axis offset tables (VolumeDesc::axis_ab / axis_z)
  ovrhip::VolumeDesc vd_replica[ovrhip::kLayouts] = {};
  // Replicas are built in the background (round 4): ovr_hip_set_volume uploads the general layout only and PLANS the others (which exist
  // for the type, fit the 40 % rule and the 32-bit in-plane offsets); a replica is allocated and re-bricked from the general layout on
  // build_stream the first time the layout rule, the tuner or a forced choice asks for it.  Every layout gives the same frame bit for bit,
  // so frames keep rendering from the general layout until the build has finished (a forced choice and the tuner's probes wait for it on the
  // device).  C3: 40 GB and four relayout passes at every ovr_hip_set_volume became 5.9 GB and one.
  //   0 = no such replica, 1 = planned (vd_replica[k] is its geometry, nothing allocated), 4 = a builder thread is allocating it and
  //   enqueueing its construction (hipMalloc of C3's 8.8 GB thin replica takes 0.25 s of HOST time: not on the render thread),
  //   2 = being built on the device (build_ev[k] pending), 3 = resident.  The builder publishes vd_replica[k] / d_replica[k] / d_axis[k]
  //   before it stores 2 (release); the render thread reads them only after it has seen 2 or 3 (acquire).
  std::atomic<int> replica_state[ovrhip::kLayouts] = {};
  std::thread builder[ovrhip::kLayouts];
  hipStream_t build_stream = nullptr;
  hipEvent_t build_ev[ovrhip::kLayouts] = {};
  int value_type = 0;
  float origin[3] = { 0, 0, 0 }, spacing[3] = { 1, 1, 1 };
  bool have_volume = false;
  float data_lower = 0.f, data_upper = 0.f; // the volume's data range as the voxel read returns it (array.cpp:297)
  float* d_data_range = nullptr;
  double upload_ms[4] = { 0, 0, 0, 0 };   // the last ovr_hip_set_volume of THIS renderer: total, allocation, copies into the device, kernels (ovr_hip_get_upload_times)
  // ovr_hip_update_volume: the staging buffer of host input (or of a device array on another GPU) - kept, only ever grown - and the last call's times
  void* d_update_stage = nullptr;
  size_t update_stage_bytes = 0;
  double update_ms[4] = { 0, 0, 0, 0 };

  // the automatic decisions (policy.hpp): layout / pipeline tuner, automatic pipeline, adaptive skipping
  ovrhip::policy::Tuner tune;
  ovrhip::policy::AutoPipeline auto_pipe;
  ovrhip::policy::Skip skip;
  bool shade_order_on = true; // OVR_HIP_SHADE_ORDER, read when the renderer is created (shade_order_params)
  float shade_beam = 32.f;    // OVR_HIP_SHADE_BEAM: voxels across a light beam

  // macrocells (empty-space skipping)
  float* d_mc_minmax = nullptr;
  float* d_mc_majorant = nullptr;
  unsigned char* d_mc_occupancy = nullptr; // coarse, dilated occupancy (skip intervals of the march)
  unsigned char* d_mc_fine = nullptr;      // per-macrocell dilated occupancy (the primary rays' refinement of those intervals)
  size_t mc_cells = 0;
  bool mc_ranges_valid = false, mc_majorant_valid = false;

  // transfer function
  float* d_tf_color = nullptr;
  float* d_tf_alpha = nullptr;   // inside d_tf_color's allocation: the colours (n_color x 4 floats), then the alphas
  float* h_tf = nullptr;         // pinned staging of both tables
  hipEvent_t ev_tf = nullptr;    // behind the last table copy
  bool tf_copy_pending = false;  // a frame has not yet been ordered behind ev_tf
  int n_color = 0, n_alpha = 0;
  bool have_tfn = false;
  unsigned long long tf_generation = 0; // + 1 with every upload of the tables (what is derived from them - the pre-integration's node table - carries it)

  // framebuffer sets
  float* d_rgba[2] = { nullptr, nullptr };
  float* d_grad[2] = { nullptr, nullptr };
  float* h_rgba[2] = { nullptr, nullptr };
  float* h_grad[2] = { nullptr, nullptr };
  // the pixel rectangle each host mirror was last refreshed in ({x0, y0, x1, y1}, empty at first): mapframe(HOST) copies only the
  // rectangle the volume's box projects into - every pixel outside it is exactly 0 on the device and stays 0 in the mirror
  int h_rgba_rect[2][4] = {}, h_grad_rect[2][4] = {};
  int d_rect[2][4] = {}; // per framebuffer set: the rectangle of the camera its last frame was rendered with (empty: never rendered, all zeros)
  float* d_accum = nullptr;
  uint32_t* d_rgba8 = nullptr; // mapframe_rgba8: device and pinned host copy of the 8-bit frame
  uint32_t* h_rgba8 = nullptr;
  uint16_t* d_rgba16f = nullptr; // mapframe_rgba16f: the half frame of the EXR writer
  uint16_t* h_rgba16f = nullptr;
  float* d_spp_rgba = nullptr; // pooled pipeline, spp > 1: sums over the sample-per-pixel generations
  float* d_spp_grad = nullptr;
  size_t fb_pixels = 0;
  int cur = 0;
  bool fb_reset = true; // the accumulation starts over with the next accumulated frame: set by apply_effects alone, consumed by the frame
  int frame_index = 0;
  bool camera_dirty = true;

  ovrhip::host::ConvergenceState conv;
  ovrhip::host::ReconstructionState recon;
  ovrhip::host::ShadowCacheState shadow_cache;

  // sparse sampling
  float* d_noise = nullptr;
  int noise_xy = 0;
  int32_t* d_sparse_xy = nullptr;
  unsigned int* d_block_counts = nullptr;
  unsigned long long* d_sparse_count = nullptr;
  size_t sparse_pixels = 0;
  unsigned long long sparse_prev_pixels = 0; // pixels of the previous sparse frame (RayMarchParams::sparse_hint_pixels)

  // counters
  unsigned long long* d_counters = nullptr;  // start of the frame words: [0, 64) the counters, [128, 128 + ctrl) the pool's control words, then the reduction's ticket
  std::atomic<bool> phase_timing{ true };    // ovr_hip_set_phase_timing (any thread)
  bool frame_phase_timed = true;             // ... as the frame in flight was launched
  bool frame_words_dirty = true;             // the next launch may not rely on the last frame's reduction having zeroed them (RayMarchParams::zero_first)
  unsigned int* d_block_counters = nullptr; // per-workgroup partial counters
  unsigned long long* d_trace = nullptr;    // OVR_HIP_TRACE=1 diagnostic buffer
  size_t trace_words = 0;
  unsigned long long* h_counters = nullptr; // pinned
  bool outside_hits = false;   // a frame of the running accumulation had a ray that hit the box from outside its silhouette (see finish_frame_one)
  int frame_set = 0;           // the framebuffer set the frame in flight renders into

  ovrhip::host::ScheduleState sched;

  // request pool of the pooled shading pipeline
  ovrhip::PoolDesc pool{};
  size_t pool_tiles = 0;
  unsigned int* h_ctrl = nullptr; // pinned copy of pool.ctrl

  ovrhip::RayMarchParams P{};
  ovrhip::LaunchPlan plan{}; // of the frame in flight (launch_frame): which kernel variants P was launched with
  ovr_hip_stats stats{};
  double render_time_ms = 0.0;
  bool async_pending = false;
  // pipelined gather (ovr_hip_pack_tiles before the frame is known to be complete): allowed while the request pool has proven
  // roomy for this configuration - the last frame since the last commit that changed anything used at most half of it
  bool pool_roomy = false;
  bool packed_early = false; // the pending frame's tiles were packed without waiting for it

  ovrhip::host::GroupState group;

  hipStream_t stream() const { return use_user_stream ? user_stream : own_stream[cur]; }
  // the whole framebuffer set `set` is mapped, not the rectangle the box projects into
  void map_whole_set(int set) { int* q = d_rect[set]; q[0] = 0; q[1] = 0; q[2] = fbsize.current.w; q[3] = fbsize.current.h; }
};

namespace ovrhip {
namespace host __attribute__((visibility("hidden"))) {

inline int set_device(ovr_hip_renderer* r) { HIP_TRY(hipSetDevice(r->device)); return 0; }
// what the committed state makes the next frame (launch_plan.hpp: slices over isovalues over a projection mode over the march)
inline ovrhip::CommittedFrame committed_frame(const ovr_hip_renderer* r)
{
  return ovrhip::committed_frame(r->slices.current.n, r->isosurfaces.current.n, r->projection.current);
}

// (see GroupState::mtx; followers are only ever called with their leader's lock held)
struct GroupLock {
  std::unique_lock<std::mutex> lk;
  explicit GroupLock(ovr_hip_renderer* r) { if (r && !r->group.leader && r->group.members.size() > 1) lk = std::unique_lock<std::mutex>(r->group.mtx); }
};

// buffers.cpp: allocation and release of everything sized by the framebuffer, the frame's work or a mode
int free_convergence(ovr_hip_renderer* r);
int ensure_convergence(ovr_hip_renderer* r, bool lists);
int free_reconstruction(ovr_hip_renderer* r);
int ensure_reconstruction(ovr_hip_renderer* r);
int free_framebuffers(ovr_hip_renderer* r);
int resize_framebuffers(ovr_hip_renderer* r, int w, int h);
int ensure_pool(ovr_hip_renderer* r, size_t chunks);
int ensure_sparse_buffers(ovr_hip_renderer* r);
void free_shadow_cache(ovr_hip_renderer* r);

// volume.cpp: what a commit or an upload derives from camera, volume, transfer function and light; the replicas.  apply_effects carries out what
// commit_plan.hpp's plan_commit asked for: fb_reset, the schedule's flags, pool_roomy, the validity flags of macrocells, lattice and estimate and the
// tuner's restart are written there and (beside the frame's own bookkeeping and the code that builds each of them) nowhere else
void apply_effects(ovr_hip_renderer* r, const ovrhip::commit::Effects& fx);
void update_camera(ovr_hip_renderer* r);
void update_volume_params(ovr_hip_renderer* r);
void apply_lighting(ovr_hip_renderer* r);
V3 unit_light(const LightP& l); // the unit vector apply_lighting derives
void apply_clip_box(ovr_hip_renderer* r);
void update_tfn_range(ovr_hip_renderer* r);
int upload_tfn(ovr_hip_renderer* r);
int update_macrocells(ovr_hip_renderer* r, hipStream_t st);
void join_builders(ovr_hip_renderer* r);
int start_replica_build(ovr_hip_renderer* r, int k, std::string* err, bool background = true);
int resolve_layout(ovr_hip_renderer* r, int choice, bool may_wait, hipStream_t st);
int poll_replica_builds(ovr_hip_renderer* r);

// frame.cpp: one renderer's frame
ovrhip::SparseMaskParams make_mask_params(ovr_hip_renderer* r, int frame_index, int32_t* out_xy);
int refresh_mirror(ovr_hip_renderer* r, float* host, const float* dev, int channels, const int dev_rect[4], int last[4], hipStream_t st);
int enqueue_frame(ovr_hip_renderer* r);
int finish_frame_one(ovr_hip_renderer* r);
// the shadow cache: the parameters the shadow march reads as the next frame would set them (general layout, sampling rate, transfer function) into q; the lattice
// the next cached frame reads bound into q - mode CACHED builds it first if it is stale, on st, and waits for it
void fill_shadow_params(ovr_hip_renderer* r, ovrhip::RayMarchParams& q);
// the macrocells' value ranges for a range-skipping projection: valid whenever a volume is resident (the upload and ovr_hip_update_volume keep them current)
const float* projection_ranges(const ovr_hip_renderer* r);
// the committed isovalues into a frame's parameters (iso_n = 0: no isosurface frame)
void fill_isosurface_params(const ovr_hip_renderer* r, ovrhip::RayMarchParams& q);
// the committed slices into a frame's parameters (slice_n = 0: no slice frame)
void fill_slice_params(const ovr_hip_renderer* r, ovrhip::RayMarchParams& q);
// the next frame is a pre-integrated march: the committed frame is the march, the committed shading mode NONE and the committed mode SEGMENTS
bool preintegrated_frame(const ovr_hip_renderer* r);
// q.preintegrated / preint_m1 / preint_nodes for the frame q describes so far (its layout, tables and clip box are bound): the node table is rebuilt when the
// transfer function was committed since, or the plan's subdivision changed.  A plan that is an error binds no table: the launch then fails as any error plan does
int bind_preintegration(ovr_hip_renderer* r, ovrhip::RayMarchParams& q);
// the next frame is a gradient-opacity march (host/gradient_opacity_host.hpp gradient_opacity_active over the committed state)
bool gradient_opacity_frame(const ovr_hip_renderer* r);
// q.gradient_opacity (on) and the committed thresholds
void fill_gradient_opacity_params(const ovr_hip_renderer* r, ovrhip::RayMarchParams& q, bool on);
// the next frame is a depth-limited march (host/max_depth_host.hpp max_depth_active over the committed state and the committed framebuffer size)
bool max_depth_frame(const ovr_hip_renderer* r);
// the next frame is a depth frame (host/depth_output_host.hpp depth_output_active over the committed state); it applies the depth limit iff max_depth_frame
bool depth_output_frame(const ovr_hip_renderer* r);
int ensure_shadow_cache(ovr_hip_renderer* r, ovrhip::RayMarchParams& q, hipStream_t st);
int shadow_lattice_dims(const ovr_hip_renderer* r, int cell, int dims[3]); // of the resident volume; EINVAL past 2^31 - 1 nodes
int shadow_lattice_positions(ovr_hip_renderer* r, const int dims[3], float* d_pos, hipStream_t st);

// group.cpp: the device group
enum { GW_NONE = 0, GW_COMMIT, GW_RENDER, GW_SHIP, GW_FINISH, GW_SWAP, GW_CALL, GW_QUIT };
int finish_frame(ovr_hip_renderer* r); // resolves the frame in flight: one renderer, or a device group incl. its gather
int group_run(ovr_hip_renderer* L, int cmd, const std::function<int()>& own = {});
int group_call(ovr_hip_renderer* L, const std::function<int(ovr_hip_renderer*)>& f, const std::function<int()>& own = {});
void group_stop_workers(ovr_hip_renderer* L);
void group_release(ovr_hip_renderer* r);

} // namespace host
} // namespace ovrhip
