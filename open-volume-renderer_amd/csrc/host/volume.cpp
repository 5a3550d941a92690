// volume.cpp - what the renderer derives from its volume, camera, transfer function and light: the frame parameters a commit refreshes, the
// macrocell grids, the volume upload and the replicas built in the background.
//   volume + TF upload ................ volume.cpp:110-179, array.cpp:287-351 (citations relative to the reference tree)
#include "state.hpp"

#include <cfloat>
#include <chrono>
#include <cstdlib>

using namespace ovrhip;
using namespace ovrhip::host;

namespace ovrhip {
namespace host {

// array.h:68-106
static float integer_normalize(float value, int type)
{
  switch (type) {
  case OVR_HIP_TYPE_UINT8: return (float)(uint8_t)value / 255.f;
  case OVR_HIP_TYPE_INT8: { const float n = (float)(int8_t)value / 127.f; return n < -1.f ? -1.f : n; }
  case OVR_HIP_TYPE_UINT16: return (float)(uint16_t)value / 65535.f;
  case OVR_HIP_TYPE_INT16: { const float n = (float)(int16_t)value / 32767.f; return n < -1.f ? -1.f : n; }
  case OVR_HIP_TYPE_UINT32: return (float)(uint32_t)value / (float)UINT32_MAX;
  case OVR_HIP_TYPE_INT32: { const float n = (float)(int32_t)value / (float)INT32_MAX; return n < -1.f ? -1.f : n; }
  default: return value;
  }
}
// the ValueType the reference's device volume ends up with (array.cpp:322-347): u16 / i16 / f64 are sampled as RAW float
static int device_value_type(int t)
{
  if (t == OVR_HIP_TYPE_UINT16 || t == OVR_HIP_TYPE_INT16 || t == OVR_HIP_TYPE_DOUBLE) return OVR_HIP_TYPE_FLOAT;
  return t;
}
static size_t value_type_size(int t)
{
  switch (t) {
  case OVR_HIP_TYPE_UINT8: case OVR_HIP_TYPE_INT8: return 1;
  case OVR_HIP_TYPE_UINT16: case OVR_HIP_TYPE_INT16: return 2;
  case OVR_HIP_TYPE_UINT32: case OVR_HIP_TYPE_INT32: case OVR_HIP_TYPE_FLOAT: return 4;
  case OVR_HIP_TYPE_DOUBLE: return 8;
  default: return 0;
  }
}

// device_impl.cpp:125-144
void update_camera(ovr_hip_renderer* r)
{
  const CameraP& c = r->camera.current;
  const int W = r->fbsize.current.w, H = r->fbsize.current.h;
  // the orthographic camera (open-volume-renderer_amd/camera.py): the same expressions with the image's world height in the tangent's place
  const bool ortho = c.kind == OVR_HIP_CAMERA_ORTHOGRAPHIC;
  const float t = ortho ? c.height : 2.f * std::tan(c.fovy * 0.5f * (float)M_PI / 180.f);
  const float aspect = (float)W / (float)H;
  const V3 from = { c.from[0], c.from[1], c.from[2] }, at = { c.at[0], c.at[1], c.at[2] }, up = { c.up[0], c.up[1], c.up[2] };
  const V3 dir = normalize(sub(at, from));
  const V3 hor = scale(t * aspect, normalize(cross(dir, up)));
  const V3 cr = cross(hor, dir);
  const V3 ver = { cr.x / aspect, cr.y / aspect, cr.z / aspect };
  RayMarchParams& P = r->P;
  P.cam_pos = { from.x, from.y, from.z };
  P.cam_dir = { dir.x, dir.y, dir.z };
  P.cam_hor = { hor.x, hor.y, hor.z };
  P.cam_ver = { ver.x, ver.y, ver.z };
  P.cam_orthographic = ortho ? 1 : 0;
  // inverse-transpose of get_xfm_world_to_camera().l (shaders_common.h:276-289; LinearSpace.h:215-224,321)
  const V3 x = normalize(hor), y = normalize(ver), zz = normalize(dir);
  const V3 z = { -zz.x, -zz.y, -zz.z };
  const V3 vx = { x.x, y.x, z.x }, vy = { x.y, y.y, z.y }, vz = { x.z, y.z, z.z };
  const float det = dot(vx, cross(vy, vz));
  const V3 c0 = cross(vy, vz), c1 = cross(vz, vx), c2 = cross(vx, vy);
  const float m[9] = { c0.x / det, c0.y / det, c0.z / det, c1.x / det, c1.y / det, c1.z / det, c2.x / det, c2.y / det, c2.z / det };
  std::memcpy(P.wtc_it, m, sizeof(m));
}

// volume.cpp:131-145 + device_impl.cpp:288-296 + volume.cpp:172-179
void update_volume_params(ovr_hip_renderer* r)
{
  RayMarchParams& P = r->P;
  const bool vertex = r->grid_convention.current == OVR_HIP_GRID_VERTEX_CENTRED;
  const int n[3] = { r->vd.nx, r->vd.ny, r->vd.nz };
  float inv[3], wp[3], cs[3], cb[3], gs[3];
  for (int k = 0; k < 3; ++k) {
    const float ext = vertex ? (float)(n[k] - 1) : (float)n[k];
    const float sc = r->spacing[k] * ext;
    inv[k] = 1.f / sc;
    wp[k] = -(inv[k] * r->origin[k]);
    cs[k] = vertex ? (float)(n[k] - 1) : (float)n[k];
    cb[k] = vertex ? 0.f : -0.5f;
    gs[k] = vertex ? 1.f / (float)(n[k] - 1) : 1.f / (float)n[k];
  }
  P.inv_scale = { inv[0], inv[1], inv[2] };
  P.wto_p = { wp[0], wp[1], wp[2] };
  P.otw_it = P.inv_scale;
  P.coord_scale = { cs[0], cs[1], cs[2] };
  P.coord_bias = { cb[0], cb[1], cb[2] };
  P.grad_step = { gs[0], gs[1], gs[2] };
  P.vol = r->vd;
  P.vol.data = r->d_volume;
  apply_clip_box(r); // the object box follows the volume's transform
}

// the committed clip box into the frame's parameters: per axis clamp01(fmaf(world, inv_scale, wto_p)) - the float constants that take a world position
// into the volume's [0, 1] box (to_object in the kernels; open-volume-renderer_amd/clipping.py object_box).  -inf / +inf clamp to 0 / 1.  Without a clip
// box, or before a volume is set, the unit cube - and clip_on = 0: the kernels of the unclipped state are launched
void apply_clip_box(ovr_hip_renderer* r)
{
  RayMarchParams& P = r->P;
  const ClipP& c = r->clip.current;
  const float inv[3] = { P.inv_scale.x, P.inv_scale.y, P.inv_scale.z }, wp[3] = { P.wto_p.x, P.wto_p.y, P.wto_p.z };
  float lo[3] = { 0.f, 0.f, 0.f }, hi[3] = { 1.f, 1.f, 1.f };
  P.clip_on = c.enabled && r->have_volume ? 1 : 0;
  if (P.clip_on)
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::fmin(std::fmax(std::fma(c.lower[k], inv[k], wp[k]), 0.f), 1.f);
      hi[k] = std::fmin(std::fmax(std::fma(c.upper[k], inv[k], wp[k]), 0.f), 1.f);
    }
  P.clip_lo = { lo[0], lo[1], lo[2] };
  P.clip_hi = { hi[0], hi[1], hi[2] };
}

V3 unit_light(const LightP& l) { return normalize({ l.dir[0], l.dir[1], l.dir[2] }); }

// the committed light and material into the frame's parameters.  The raw vector is normalised here, by the routine that normalised the reference's
// literal when the light was one: the same raw vector gives the same unit vector as the CPU oracle's (shade_order_params reads it per frame)
void apply_lighting(ovr_hip_renderer* r)
{
  RayMarchParams& P = r->P;
  const LightP& l = r->light.current;
  const MaterialP& m = r->material.current;
  const V3 L = unit_light(l);
  P.light = { L.x, L.y, L.z };
  P.light_i2 = 2.f * l.intensity;
  P.mat_ka = m.ambient; P.mat_kd = m.diffuse; P.mat_ks = m.specular; P.mat_shininess = m.shininess;
}

// carries out a plan (commit_plan.hpp).  The four kFree* effects are not here: a free can fail, so the commit runs them where it consumes the value
void apply_effects(ovr_hip_renderer* r, const commit::Effects& fx)
{
  using namespace commit;
  if (fx.has(kCameraParams)) { update_camera(r); r->camera_dirty = false; }
  if (fx.has(kVolumeParams)) update_volume_params(r); // (and the clip box: the object box follows the volume's transform)
  if (fx.has(kLighting)) apply_lighting(r);
  if (fx.has(kClipParams)) apply_clip_box(r);
  if (fx.has(kResort)) r->sched.dirty = true;
  if (fx.has(kRelist)) r->sched.list_dirty = true;
  if (fx.has(kBumpClearGen)) r->sched.clear_gen++;
  if (fx.has(kPoolUnproven)) r->pool_roomy = false;
  if (fx.has(kRangesVoid)) r->mc_ranges_valid = false;
  if (fx.has(kMajorantVoid)) r->mc_majorant_valid = false;
  if (fx.has(kSkipRestart)) r->skip.restart();
  if (fx.has(kLatticeStale)) r->shadow_cache.built_valid = false;
  switch (fx.tuner) {
  case kTunerKeeps: break;
  case kTunerCameraMoved: r->tune.configuration_changed(true); break;
  case kTunerStateZero: r->tune.state = 0; break;
  case kTunerChanged: r->tune.configuration_changed(false); break;
  case kTunerVoid: r->tune.restart(); break;
  }
  if (fx.has(kReset)) r->fb_reset = true;
  if (fx.has(kEstimateVoid)) { r->conv.valid = false; r->conv.retired = 0; r->conv.active = r->sched.n_work; }
}

// StructuredRegularVolume::set_value_range (volume.cpp:131-145): a valid range replaces the one in effect, an invalid one
// (hi < lo, the default (1, -1)) keeps it - after a volume load that is the data range (array.cpp:297, volume.cpp:187-191)
void update_tfn_range(ovr_hip_renderer* r)
{
  RayMarchParams& P = r->P;
  const int dt = device_value_type(r->value_type);
  const TfnP& t = r->tfn.current;
  if (t.hi >= t.lo) { // volume.cpp:135
    P.tf_upper = integer_normalize(t.hi, dt);
    P.tf_lower = integer_normalize(t.lo, dt);
  }
  // a degenerate range (upper == lower: a constant volume under the data-range fallback) gives the reference scale = inf and the
  // coordinate clamp01((lower - lower) * inf) = clamp01(NaN) = 0 for every sample; scale = 0 yields the same 0 without a NaN
  // ever reaching a transfer-function lookup
  P.tf_scale = P.tf_upper == P.tf_lower ? 0.f : 1.f / (P.tf_upper - P.tf_lower);
}

int upload_tfn(ovr_hip_renderer* r)
{
  const TfnP& t = r->tfn.current;
  const int nc = (int)(t.colors.size() / 3), na = (int)(t.alphas.size() / 2);
  if (nc == 0 || na == 0) return 0; // volume.cpp:125: nothing happens for an empty TF
  // One pinned staging buffer, one device buffer (colours, then alphas), ONE stream-ordered copy on the render stream: the frames that read the
  // tables are enqueued behind it, the frame before it has been resolved by the commit.  (Until round 4: hipDeviceSynchronize and two
  // synchronous copies from pageable vectors - 60 of the 105 us a transfer-function edit cost beside its frame, `tools/tf_edit_time.py`.)
  const size_t words = (size_t)nc * 4 + (size_t)na;
  if (r->n_color != nc || r->n_alpha != na) {
    HIP_TRY(hipDeviceSynchronize()); // nothing may still read (or be copying into) the old tables
    if (r->d_tf_color) HIP_TRY(hipFree(r->d_tf_color));
    if (r->h_tf) HIP_TRY(hipHostFree(r->h_tf));
    r->d_tf_color = r->d_tf_alpha = nullptr; r->h_tf = nullptr;
    r->n_color = r->n_alpha = 0;
    HIP_TRY(hipMalloc((void**)&r->d_tf_color, words * sizeof(float)));
    HIP_TRY(hipHostMalloc((void**)&r->h_tf, words * sizeof(float), hipHostMallocDefault));
    r->d_tf_alpha = r->d_tf_color + (size_t)nc * 4;
    r->n_color = nc;
    r->n_alpha = na;
  }
  // (a copy of an earlier commit that has not run yet would read this buffer while it is rewritten - and be overwritten by this commit's copy, which
  // is enqueued behind it, before any frame reads the tables)
  float* c4 = r->h_tf;
  float* a = r->h_tf + (size_t)nc * 4;
  for (int i = 0; i < nc; ++i) { // volume.cpp:112-118
    c4[4 * i + 0] = t.colors[3 * i + 0];
    c4[4 * i + 1] = t.colors[3 * i + 1];
    c4[4 * i + 2] = t.colors[3 * i + 2];
    c4[4 * i + 3] = 1.f;
  }
  for (int i = 0; i < na; ++i) a[i] = t.alphas[2 * i + 1]; // volume.cpp:120-123
  HIP_TRY(hipMemcpyAsync(r->d_tf_color, r->h_tf, words * sizeof(float), hipMemcpyHostToDevice, r->stream()));
  // the next frame may run on the other framebuffer set's stream (a swap in between: renderapp's order): it waits for this event
  if (!r->ev_tf) HIP_TRY(hipEventCreateWithFlags(&r->ev_tf, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(r->ev_tf, r->stream()));
  r->tf_copy_pending = true;
  r->have_tfn = true;
  r->tf_generation++;
  return 0;
}

// the macrocell value ranges (sp.compute_value_range at load, volume.cpp:234-237): once per volume
static int update_macrocell_ranges(ovr_hip_renderer* r, hipStream_t st)
{
  const size_t cells = (size_t)((r->vd.nx + 15) / 16) * ((r->vd.ny + 15) / 16) * ((r->vd.nz + 15) / 16);
  if (cells != r->mc_cells || !r->d_mc_minmax) {
    HIP_TRY(hipDeviceSynchronize());
    if (r->d_mc_minmax) HIP_TRY(hipFree(r->d_mc_minmax));
    if (r->d_mc_majorant) HIP_TRY(hipFree(r->d_mc_majorant));
    if (r->d_mc_occupancy) HIP_TRY(hipFree(r->d_mc_occupancy));
    if (r->d_mc_fine) HIP_TRY(hipFree(r->d_mc_fine));
    r->d_mc_fine = nullptr;
    r->d_mc_minmax = r->d_mc_majorant = nullptr;
    r->d_mc_occupancy = nullptr;
    r->mc_cells = 0;
    HIP_TRY(hipMalloc((void**)&r->d_mc_minmax, cells * 2 * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&r->d_mc_majorant, cells * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&r->d_mc_occupancy, cells));
    HIP_TRY(hipMalloc((void**)&r->d_mc_fine, cells));
    r->mc_cells = cells;
    r->mc_ranges_valid = r->mc_majorant_valid = false;
  }
  if (!r->mc_ranges_valid) {
    VolumeDesc vd = r->vd;
    vd.data = r->d_volume;
    HIP_TRY(launch_macrocell_ranges(vd, r->d_mc_minmax, st));
    r->mc_ranges_valid = true;
    r->mc_majorant_valid = false;
  }
  return 0;
}

// (re)build the majorant grids when empty-space skipping is on: per TF / range change
int update_macrocells(ovr_hip_renderer* r, hipStream_t st)
{
  if (int e = update_macrocell_ranges(r, st)) return e;
  const size_t cells = r->mc_cells;
  if (!r->mc_majorant_valid) {
    // tfn.value_range / range_rcp_norm of the reference (volume.cpp:147-153) - the TF range, normalised like the data
    HIP_TRY(launch_macrocell_majorants(r->d_mc_minmax, (unsigned int)cells, r->d_tf_alpha, r->n_alpha, r->P.tf_lower, r->P.tf_upper, r->d_mc_majorant, st));
    HIP_TRY(launch_macrocell_coarse(r->d_mc_majorant, r->vd.nx, r->vd.ny, r->vd.nz, r->d_mc_occupancy, r->d_mc_fine, st));
    r->mc_majorant_valid = true;
  }
  return 0;
}

// ---- replicas built in the background (see replica_state)
void join_builders(ovr_hip_renderer* r)
{
  for (int k = 0; k < kLayouts; ++k)
    if (r->builder[k].joinable()) r->builder[k].join();
}

static void drop_replica(ovr_hip_renderer* r, int k)
{
  if (k == LAYOUT_GENERAL) return;
  if (r->builder[k].joinable()) r->builder[k].join();
  if (r->d_replica[k]) { (void)hipFree(r->d_replica[k]); r->volume_bytes -= (size_t)r->vd_replica[k].bytes; }
  if (r->d_axis[k]) (void)hipFree(r->d_axis[k]);
  r->d_replica[k] = nullptr; r->d_axis[k] = nullptr;
  r->replica_state[k] = 0;
}

// allocate replica k and enqueue its construction from the general layout on build_stream (host work: on the calling thread); on an
// allocation failure the replica is given up (an optimisation: the general layout renders the same frames) and `err` says why.
// Expects replica_state[k] == 4 (claimed); leaves 2 (enqueued) or 0 (given up).
static void build_replica_host(ovr_hip_renderer* r, int k, std::string* err)
{
  (void)hipSetDevice(r->device);
  VolumeDesc t = r->vd_replica[k];
  void *d_data = nullptr, *d_tab = nullptr;
  hipError_t e = hipMalloc(&d_data, (size_t)t.bytes + 64); // + slack: the pair load of the very last element
  if (e == hipSuccess) e = hipMalloc(&d_tab, axis_table_bytes(t));
  if (e == hipSuccess) {
    t.data = d_data;
    // padding voxels are never sampled, but must be finite: the build writes them itself (launch_relayout), only the slack is set here
    if (getenv("OVR_HIP_POISON_ALLOC") && atoi(getenv("OVR_HIP_POISON_ALLOC")) != 0) e = hipMemsetAsync(d_data, 0xff, (size_t)t.bytes, r->build_stream);
    if (e == hipSuccess) e = hipMemsetAsync((char*)d_data + (size_t)t.bytes, 0, 64, r->build_stream);
  }
  if (e == hipSuccess) e = launch_axis_tables(t, d_tab, r->build_stream);
  if (e == hipSuccess) {
    VolumeDesc g = r->vd_replica[LAYOUT_GENERAL];
    g.data = r->d_volume;
    e = launch_rebrick(g, d_data, t, r->build_stream);
  }
  if (e == hipSuccess) e = hipEventRecord(r->build_ev[k], r->build_stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(r->build_stream);
    if (err) *err = hipGetErrorString(e);
    if (d_data) (void)hipFree(d_data);
    if (d_tab) (void)hipFree(d_tab);
    r->replica_state[k].store(0, std::memory_order_release);
    return;
  }
  r->vd_replica[k] = t;
  r->d_replica[k] = d_data;
  r->d_axis[k] = d_tab;
  r->volume_bytes += (size_t)t.bytes;
  r->replica_state[k].store(2, std::memory_order_release);
}

// a planned replica is wanted: in the background (a builder thread does the host work; frames go on from the general layout) or at once
int start_replica_build(ovr_hip_renderer* r, int k, std::string* err, bool background)
{
  int planned = 1;
  if (!r->replica_state[k].compare_exchange_strong(planned, 4)) return 0; // not planned, or already on its way
  if (r->builder[k].joinable()) r->builder[k].join();
  static const bool threads = !(getenv("OVR_HIP_BUILD_THREAD") && atoi(getenv("OVR_HIP_BUILD_THREAD")) == 0); // measurements: 0 = host work on the caller
  bool started = false;
  if (background && threads) {
    try { r->builder[k] = std::thread(build_replica_host, r, k, nullptr); started = true; }
    catch (const std::exception&) { started = false; } // no thread to be had: the caller does the host work
  }
  if (!started) build_replica_host(r, k, err);
  return 0;
}

// the layout a frame on stream `st` reads when it asks for `choice`: the replica if it is resident; if it is still being built, the replica
// when the frame may wait for it (forced choice), else the general layout (same frame bit for bit)
int resolve_layout(ovr_hip_renderer* r, int choice, bool may_wait, hipStream_t st)
{
  if (choice <= LAYOUT_GENERAL || choice >= kLayouts || r->replica_state[choice].load(std::memory_order_acquire) == 0) return LAYOUT_GENERAL;
  if (r->replica_state[choice] == 1) (void)start_replica_build(r, choice, nullptr, !may_wait);
  if (r->replica_state[choice] == 4 && may_wait && r->builder[choice].joinable()) r->builder[choice].join(); // the host part of the build
  int state = r->replica_state[choice].load(std::memory_order_acquire);
  if (state == 2 && hipEventQuery(r->build_ev[choice]) == hipSuccess) { r->replica_state[choice] = 3; state = 3; }
  if (state == 3) return choice;
  if (state == 2 && may_wait && hipStreamWaitEvent(st, r->build_ev[choice], 0) == hipSuccess) return choice;
  (void)hipGetLastError();
  return LAYOUT_GENERAL;
}
// the replicas whose build the device has finished become resident; returns how many are still being built (by a builder thread or on the
// device).  hipEventQuery leaves hipErrorNotReady behind: each caller swallows it where it always did
int poll_replica_builds(ovr_hip_renderer* r)
{
  int building = 0;
  for (int k = 1; k < kLayouts; ++k) {
    int state = r->replica_state[k].load(std::memory_order_acquire);
    if (state == 2 && hipEventQuery(r->build_ev[k]) == hipSuccess) { r->replica_state[k] = 3; state = 3; }
    if (state == 2 || state == 4) building++;
  }
  return building;
}

static double ms_since(std::chrono::high_resolution_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count(); }

// The other layouts (ovr_hip_kernels.h: thin replicas for views along a volume axis, the quad replica for frames that shade every sample) are
// only PLANNED here and built in the background when a frame first asks for one (replica_state).  mode 1 (default): planned when the type has
// them and they fit comfortably (all replicas <= 40 % of the free HBM); mode 2: all of them, built before this call returns (an allocation
// failure is an error); mode 0: none.  OVR_HIP_QUAD=0 leaves the quad replica out (measurements).
static int plan_replicas(ovr_hip_renderer* r, int vt, const VolumeDesc& vd)
{
  {
    std::lock_guard<std::mutex> lk(r->mtx);
    (void)r->layouts.update();
  }
  {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    double planned = 0.0;
    // false: the type has no such replica (nothing is planned from a VolumeDesc that volume_layout did not fill)
    auto plan = [&](int k, VolumeDesc& t) { t = vd; t.data = nullptr; t.axis_ab = nullptr; t.axis_z = nullptr; return volume_layout(replica_voxel_type(vt, k), vd.nx, vd.ny, vd.nz, t); };
    if (r->layouts.current != 0 && replica_voxel_type(vt, LAYOUT_THIN) >= 0) {
      VolumeDesc t1, t2;
      if (plan(LAYOUT_THIN, t1) && plan(LAYOUT_THIN_T, t2) && layout_offsets_fit(t1) && layout_offsets_fit(t2) && (r->layouts.current == 2 || (double)(t1.bytes + t2.bytes) <= 0.4 * (double)free_b)) {
        r->vd_replica[LAYOUT_THIN] = t1; r->vd_replica[LAYOUT_THIN_T] = t2;
        r->replica_state[LAYOUT_THIN] = r->replica_state[LAYOUT_THIN_T] = 1;
        planned += (double)(t1.bytes + t2.bytes);
      }
      else if (r->layouts.current == 2) return fail(OVR_HIP_EINVAL, "[hip] volume replicas requested (layouts mode 2) but one z layer of a thin replica exceeds 2^32 elements");
    }
    static const bool want_quad = !(getenv("OVR_HIP_QUAD") && atoi(getenv("OVR_HIP_QUAD")) == 0);
    if (want_quad && r->layouts.current != 0 && replica_voxel_type(vt, LAYOUT_QUAD) >= 0) {
      VolumeDesc tq;
      if (plan(LAYOUT_QUAD, tq) && layout_offsets_fit(tq) && (r->layouts.current == 2 || (double)tq.bytes + planned <= 0.4 * (double)free_b)) {
        r->vd_replica[LAYOUT_QUAD] = tq;
        r->replica_state[LAYOUT_QUAD] = 1;
      }
    }
  }
  return 0;
}

struct UploadTimes { double alloc = 0.0, copy = 0.0, kern = 0.0; }; // milliseconds: allocation, copies into the device, kernels

// the caller's voxels into the general layout (r->d_replica[0]), re-bricked on the device; t_seg = when the kernels' share of the time began
static int upload_voxels(ovr_hip_renderer* r, const void* data, int mem_kind, int value_type, std::chrono::high_resolution_clock::time_point t_seg, UploadTimes& t)
{
  const VolumeDesc& vd = r->vd_replica[0];
  hipStream_t st = r->own_stream[0];
  auto relayout_all = [&](const void* src, int z0, int nzc) -> hipError_t {
    return launch_relayout(src, value_type, r->d_replica[0], r->vd_replica[0], z0, nzc, st);
  };

  const size_t in_es = value_type_size(value_type);
  const size_t slice_bytes = (size_t)vd.nx * vd.ny * in_es;
  int src_device = r->device; // a device array may live on another GPU (a device group's followers): staged through peer copies
  if (mem_kind == OVR_HIP_MEM_DEVICE) {
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, data) == hipSuccess) src_device = attr.device;
    else (void)hipGetLastError();
  }
  if (mem_kind == OVR_HIP_MEM_DEVICE && src_device == r->device) {
    // chunk over z only to keep grid.z within limits
    for (int z0 = 0; z0 < vd.nz; z0 += 32768) {
      const int nzc = std::min(32768, vd.nz - z0);
      HIP_TRY(relayout_all((const char*)data + (size_t)z0 * slice_bytes, z0, nzc));
    }
    HIP_TRY(hipStreamSynchronize(st));
    t.kern += ms_since(t_seg);
  }
  else {
    // host input: staged through a bounded device buffer (<= 1 GiB), slab by slab
    size_t slab = std::max<size_t>(1, ((size_t)1 << 30) / std::max<size_t>(1, slice_bytes));
    slab = std::min<size_t>(slab, (size_t)vd.nz);
    void* d_stage = nullptr;
    t_seg = std::chrono::high_resolution_clock::now();
    HIP_TRY(hipMalloc(&d_stage, slab * slice_bytes));
    t.alloc += ms_since(t_seg);
    for (int z0 = 0; z0 < vd.nz; z0 += (int)slab) {
      const int nzc = (int)std::min<size_t>(slab, (size_t)(vd.nz - z0));
      t_seg = std::chrono::high_resolution_clock::now();
      hipError_t e = mem_kind == OVR_HIP_MEM_DEVICE
                         ? hipMemcpyPeerAsync(d_stage, r->device, (const char*)data + (size_t)z0 * slice_bytes, src_device, (size_t)nzc * slice_bytes, st)
                         : hipMemcpyAsync(d_stage, (const char*)data + (size_t)z0 * slice_bytes, (size_t)nzc * slice_bytes, hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st); // (the slab is waited for before its re-bricking starts: the split of the upload time is exact, and
      t.copy += ms_since(t_seg);                          // the next copy could not overlap the kernel anyway - it writes the one staging buffer the kernel reads)
      t_seg = std::chrono::high_resolution_clock::now();
      if (e == hipSuccess) e = relayout_all(d_stage, z0, nzc);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      t.kern += ms_since(t_seg);
      if (e != hipSuccess) { (void)hipFree(d_stage); return fail(OVR_HIP_EDEVICE, std::string("[hip] volume upload failed: ") + hipGetErrorString(e)); }
    }
    HIP_TRY(hipFree(d_stage));
  }
  return 0;
}

// one renderer's volume upload (a group member's or a single renderer's).  r->upload_ms = { total, allocation, host-to-device / peer copies, kernels }
static int set_volume_one(ovr_hip_renderer* r, const void* data, int mem_kind, int value_type, const int32_t dims[3],
                          const float grid_origin[3], const float grid_spacing[3])
{
  const auto t_call = std::chrono::high_resolution_clock::now();
  UploadTimes t;
  if (!r || !data || !dims || !grid_origin || !grid_spacing) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_volume: null argument");
  for (double& v : r->upload_ms) v = 0.0;
  if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_volume: dims must be positive");
  const int vt = device_voxel_type(value_type);
  if (vt < 0) return fail(OVR_HIP_EINVAL, "[Optix7] unexpected volume type ..."); // array.cpp:348, same text
  if (mem_kind != OVR_HIP_MEM_HOST && mem_kind != OVR_HIP_MEM_DEVICE) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_volume: bad mem_kind");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame_one(r)) return e;
  HIP_TRY(hipDeviceSynchronize());

  hipStream_t st = r->own_stream[0];
  VolumeDesc vd{};
  if (!volume_layout(vt, dims[0], dims[1], dims[2], vd)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_volume: no layout for this voxel type");
  vd.value_scale = 1.f;
  vd.value_min_clamp = -FLT_MAX;
  if (vt == VOX_U8) vd.value_scale = 1.f / 255.f;
  if (vt == VOX_I8) { vd.value_scale = 1.f / 127.f; vd.value_min_clamp = -127.f; }
  const size_t bytes = (size_t)vd.bytes;
  if (!layout_offsets_fit(vd))
    return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_volume: one z layer of the volume exceeds 2^32 stored voxels (x * y too large for the 32-bit in-plane offsets)");

  auto t_seg = std::chrono::high_resolution_clock::now();
  join_builders(r);                               // a builder thread may still be enqueueing a replica of the OLD volume
  HIP_TRY(hipStreamSynchronize(r->build_stream)); // ... which reads the old general layout
  for (int k = 0; k < kLayouts; ++k) {
    if (r->d_replica[k]) HIP_TRY(hipFree(r->d_replica[k]));
    r->d_replica[k] = nullptr;
    if (r->d_axis[k]) HIP_TRY(hipFree(r->d_axis[k]));
    r->d_axis[k] = nullptr;
    r->vd_replica[k] = VolumeDesc{};
    r->replica_state[k] = 0;
  }
  r->d_volume = nullptr;
  r->have_volume = false; // until the new one is completely resident: a failure below must not leave a half-built volume renderable
  HIP_TRY(hipMalloc(&r->d_replica[0], bytes + 64)); // + slack: the pair load of the very last element
  // (tests: OVR_HIP_POISON_ALLOC=1 fills a fresh layout with 0xff bytes - NaN / the type's extreme - first: a padding element the build left out would show)
  if (getenv("OVR_HIP_POISON_ALLOC") && atoi(getenv("OVR_HIP_POISON_ALLOC")) != 0) HIP_TRY(hipMemsetAsync(r->d_replica[0], 0xff, bytes, st));
  HIP_TRY(hipMemsetAsync((char*)r->d_replica[0] + bytes, 0, 64, st)); // the slack; the relayout launches write every element of the layout itself, padding included
  r->d_volume = r->d_replica[0];
  r->volume_bytes = bytes;
  vd.data = r->d_volume;
  r->vd_replica[0] = vd;
  r->replica_state[0] = 3;
  if (int e = plan_replicas(r, vt, vd)) return e;
  HIP_TRY(hipMalloc(&r->d_axis[0], axis_table_bytes(r->vd_replica[0]))); // the layout's per-axis offset tables, staged into LDS by every march / shade workgroup
  // (allocation: a FRESH hipMalloc costs 30-60 ms per GiB on this platform - the driver maps and clears the pages - and microseconds when the runtime
  // still holds a freed block of that size: C4's 21.5 GB layout is 0.5-1.2 s in a new process, 0.1 ms on the next upload; tools/malloc_time.cpp)
  t.alloc += ms_since(t_seg);
  t_seg = std::chrono::high_resolution_clock::now();
  HIP_TRY(launch_axis_tables(r->vd_replica[0], r->d_axis[0], st));
  vd = r->vd_replica[0];
  if (int e = upload_voxels(r, data, mem_kind, value_type, t_seg, t)) return e;
  t_seg = std::chrono::high_resolution_clock::now();
  r->vd = vd;
  if (r->layouts.current == 2) { // all planned replicas now, before the call returns
    for (int k = 1; k < kLayouts; ++k) {
      if (r->replica_state[k] != 1) continue;
      std::string err;
      (void)start_replica_build(r, k, &err, false);
      if (r->replica_state[k] != 2) {
        for (int j = 1; j < kLayouts; ++j) drop_replica(r, j);
        return fail(OVR_HIP_EDEVICE, std::string("[hip] volume replicas requested (layouts mode 2) but their allocation failed: ") + err);
      }
    }
    HIP_TRY(hipStreamSynchronize(r->build_stream));
    for (int k = 1; k < kLayouts; ++k)
      if (r->replica_state[k] == 2) r->replica_state[k] = 3;
  }
  r->value_type = value_type;
  std::memcpy(r->origin, grid_origin, sizeof(r->origin));
  std::memcpy(r->spacing, grid_spacing, sizeof(r->spacing));
  r->have_volume = true;
  {
    commit::Changes ch;
    ch.happened(commit::kVolumeUpload);
    commit::CommitFacts facts;
    facts.volume = true;
    apply_effects(r, commit::plan_commit(ch, facts)); // (a pooled frame of THIS volume has to prove the pool: ovr_hip_pack_tiles packs early only then)
  }
  // load_from_array3d_scalar (volume.cpp:181-191, 234-237): the macrocell value ranges and, from them, the data range the
  // reference finds with compute_scalar_range (array.cpp:27-66,297) - it is the transfer-function range until a valid one is set
  if (int e = update_macrocell_ranges(r, st)) return e;
  HIP_TRY(launch_minmax_reduce(r->d_mc_minmax, (unsigned long long)r->mc_cells, r->d_data_range, st));
  float dr[2] = { 0.f, 0.f };
  HIP_TRY(hipMemcpyAsync(dr, r->d_data_range, sizeof(dr), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  r->data_lower = dr[0];
  r->data_upper = dr[1];
  r->P.tf_lower = dr[0];
  r->P.tf_upper = dr[1];
  update_tfn_range(r);
  t.kern += ms_since(t_seg); // mode-2 replica builds, macrocell ranges, the data range
  r->upload_ms[0] = ms_since(t_call); r->upload_ms[1] = t.alloc; r->upload_ms[2] = t.copy; r->upload_ms[3] = t.kern;
  return 0;
}

// one renderer's ovr_hip_update_volume (a group member's or a single renderer's); the arguments have been checked.  r->update_ms like r->upload_ms
static int update_volume_one(ovr_hip_renderer* r, const void* data, int mem_kind, int value_type, const int32_t lower[3], const int32_t extent[3])
{
  const auto t_call = std::chrono::high_resolution_clock::now();
  UploadTimes t;
  for (double& v : r->update_ms) v = 0.0;
  if (int e = set_device(r)) return e;
  if (int e = finish_frame_one(r)) return e; // the frame in flight was the last reader of the layouts: nothing else is drained
  hipStream_t st = r->own_stream[0];
  update::Box box;
  for (int k = 0; k < 3; ++k) { box.lo[k] = lower[k]; box.hi[k] = lower[k] + extent[k]; }

  // a replica's build must never read a half-written general layout: the host part of every build ends here, the device part is waited for by
  // the update's stream (a replica that is only planned needs nothing - its build will read the updated layout)
  join_builders(r);
  for (int k = 1; k < kLayouts; ++k)
    if (r->replica_state[k].load(std::memory_order_acquire) == 2) HIP_TRY(hipStreamWaitEvent(st, r->build_ev[k], 0));

  const size_t in_es = value_type_size(value_type);
  const size_t slice_bytes = (size_t)extent[0] * (size_t)extent[1] * in_es;
  int src_device = r->device;
  if (mem_kind == OVR_HIP_MEM_DEVICE) {
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, data) == hipSuccess) src_device = attr.device;
    else (void)hipGetLastError();
  }
  const bool direct = mem_kind == OVR_HIP_MEM_DEVICE && src_device == r->device;
  size_t slab = (size_t)extent[2];
  if (!direct) { // staged like upload_voxels: slabs of <= 1 GiB through the renderer's buffer
    slab = std::min<size_t>(std::max<size_t>(1, ((size_t)1 << 30) / std::max<size_t>(1, slice_bytes)), (size_t)extent[2]);
    if (r->update_stage_bytes < slab * slice_bytes) {
      const auto t_seg = std::chrono::high_resolution_clock::now();
      if (r->d_update_stage) HIP_TRY(hipFree(r->d_update_stage)); // (idle: every update ends with its stream drained)
      r->d_update_stage = nullptr; r->update_stage_bytes = 0;
      HIP_TRY(hipMalloc(&r->d_update_stage, slab * slice_bytes));
      r->update_stage_bytes = slab * slice_bytes;
      t.alloc += ms_since(t_seg);
    }
  }
  // from here on the layouts are being written: a device failure leaves a volume that is neither the old nor the new one
  auto write = [&]() -> int {
    for (int z0 = 0; z0 < extent[2]; z0 += (int)slab) {
      const int nzc = (int)std::min<size_t>(slab, (size_t)(extent[2] - z0));
      const void* src = (const char*)data + (size_t)z0 * slice_bytes;
      auto t_seg = std::chrono::high_resolution_clock::now();
      if (!direct) {
        HIP_TRY(mem_kind == OVR_HIP_MEM_DEVICE ? hipMemcpyPeerAsync(r->d_update_stage, r->device, src, src_device, (size_t)nzc * slice_bytes, st)
                                               : hipMemcpyAsync(r->d_update_stage, src, (size_t)nzc * slice_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        t.copy += ms_since(t_seg);
        t_seg = std::chrono::high_resolution_clock::now();
        src = r->d_update_stage;
      }
      update::Box part = box;
      part.lo[2] = box.lo[2] + z0; part.hi[2] = part.lo[2] + nzc;
      HIP_TRY(launch_update_general(src, value_type, r->d_replica[0], r->vd_replica[0], part, st));
      if (!direct) HIP_TRY(hipStreamSynchronize(st)); // the next slab's copy overwrites what this kernel reads
      t.kern += ms_since(t_seg);
    }
    const auto t_seg = std::chrono::high_resolution_clock::now();
    VolumeDesc g = r->vd_replica[LAYOUT_GENERAL];
    g.data = r->d_volume;
    for (int k = 1; k < kLayouts; ++k) {
      const int state = r->replica_state[k].load(std::memory_order_acquire);
      if (state == 2 || state == 3) HIP_TRY(launch_update_replica(g, r->d_replica[k], r->vd_replica[k], box, st));
    }
    // the macrocells whose window meets the box, then the data range over all of them - and what ovr_hip_set_volume derives from it
    const int dims[3] = { r->vd.nx, r->vd.ny, r->vd.nz };
    VolumeDesc vd = r->vd;
    vd.data = r->d_volume;
    HIP_TRY(launch_macrocell_ranges_box(vd, r->d_mc_minmax, update::macrocell_range(dims, box), st));
    HIP_TRY(launch_minmax_reduce(r->d_mc_minmax, (unsigned long long)r->mc_cells, r->d_data_range, st));
    float dr[2] = { 0.f, 0.f };
    HIP_TRY(hipMemcpyAsync(dr, r->d_data_range, sizeof(dr), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st)); // the update is resident; frames on any stream are enqueued behind it
    r->data_lower = dr[0];
    r->data_upper = dr[1];
    r->P.tf_lower = dr[0];
    r->P.tf_upper = dr[1];
    update_tfn_range(r);
    t.kern += ms_since(t_seg);
    return 0;
  };
  if (!r->d_mc_minmax || !r->mc_ranges_valid) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_update_volume: the resident volume has no macrocell ranges");
  if (int e = write()) {
    r->have_volume = false;
    return e;
  }
  commit::Changes ch;
  ch.happened(commit::kVolumeUpdate); // (the majorants are rebuilt whole with the next frame that skips; that restarts the adaptive-skipping probe, policy::Skip)
  commit::CommitFacts facts;
  facts.volume = true;
  apply_effects(r, commit::plan_commit(ch, facts));
  r->update_ms[0] = ms_since(t_call); r->update_ms[1] = t.alloc; r->update_ms[2] = t.copy; r->update_ms[3] = t.kern;
  return 0;
}

} // namespace host
} // namespace ovrhip

extern "C" {

int ovr_hip_update_volume(ovr_hip_renderer* r, const void* data, int mem_kind, int value_type, const int32_t lower[3], const int32_t extent[3])
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_update_volume: null argument");
  if (!r->have_volume && data && lower && extent) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_update_volume: no volume is set");
  // checked once, on the handle the caller holds, before anything is posted to a member
  const int dims[3] = { r->vd.nx, r->vd.ny, r->vd.nz };
  if (const int rule = update::check_arguments(data, lower, extent, mem_kind, value_type, r->value_type, dims))
    return fail(OVR_HIP_EINVAL, std::string("[hip] ovr_hip_update_volume: ") + update::check_text(rule));
  if (r->group.members.size() <= 1) return update_volume_one(r, data, mem_kind, value_type, lower, extent);
  const auto t0 = std::chrono::high_resolution_clock::now();
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  const int e = group_call(r, [=](ovr_hip_renderer* m) { return update_volume_one(m, data, mem_kind, value_type, lower, extent); },
                           [&] { return update_volume_one(r, data, mem_kind, value_type, lower, extent); });
  if (e) {
    const std::string msg = g_last_error;
    for (ovr_hip_renderer* m : r->group.members) m->have_volume = false;
    return fail(e, msg + " (device group: the update failed on a member - no member keeps a volume)");
  }
  r->group.update_ms = ms_since(t0);
  return 0;
}

int ovr_hip_get_update_times(const ovr_hip_renderer* r, double out_ms[4])
{
  if (!r || !out_ms) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_update_times: null argument");
  for (int i = 0; i < 4; ++i) out_ms[i] = r->update_ms[i];
  if (r->group.members.size() > 1) out_ms[0] = r->group.update_ms;
  return 0;
}

int ovr_hip_get_volume_layout(ovr_hip_renderer* r, int32_t member, int32_t layout, void* host, size_t capacity_bytes, uint64_t* bytes)
{
  if (!r || !bytes) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_volume_layout: null argument");
  const size_t members = std::max<size_t>(r->group.members.size(), 1);
  if (member < 0 || (size_t)member >= members || layout < 0 || layout >= kLayouts) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_volume_layout: no such member or layout");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  ovr_hip_renderer* m = members > 1 ? r->group.members[(size_t)member] : r;
  if (!m->have_volume) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_volume_layout: no volume is set");
  if (m->builder[layout].joinable()) m->builder[layout].join();
  const int state = m->replica_state[layout].load(std::memory_order_acquire);
  if (state != 2 && state != 3) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_volume_layout: that layout is not resident");
  *bytes = (uint64_t)m->vd_replica[layout].bytes;
  if (!host) return 0;
  if (capacity_bytes < (size_t)*bytes) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_volume_layout: output too small");
  if (int e = set_device(m)) return e;
  hipError_t err = state == 2 ? hipEventSynchronize(m->build_ev[layout]) : hipSuccess;
  if (err == hipSuccess) err = hipMemcpy(host, m->d_replica[layout], (size_t)*bytes, hipMemcpyDeviceToHost);
  (void)set_device(r);
  if (err != hipSuccess) return fail(OVR_HIP_EDEVICE, std::string("[hip] ovr_hip_get_volume_layout: ") + hipGetErrorString(err));
  if (state == 2) m->replica_state[layout] = 3;
  return 0;
}

int ovr_hip_set_volume(ovr_hip_renderer* r, const void* data, int mem_kind, int value_type, const int32_t dims[3],
                       const float grid_origin[3], const float grid_spacing[3])
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_volume: null argument");
  if (r->group.members.size() <= 1) return set_volume_one(r, data, mem_kind, value_type, dims, grid_origin, grid_spacing);
  // a device group: the volume is replicated - every member uploads on its own thread, side by side (a device array is staged to the other
  // devices by peer copies).  A failure on ANY member leaves no member renderable: the members must never render different volumes
  const auto t0 = std::chrono::high_resolution_clock::now();
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  const int e = group_call(r, [=](ovr_hip_renderer* m) { return set_volume_one(m, data, mem_kind, value_type, dims, grid_origin, grid_spacing); },
                           [&] { return set_volume_one(r, data, mem_kind, value_type, dims, grid_origin, grid_spacing); });
  if (e) {
    const std::string msg = g_last_error;
    for (ovr_hip_renderer* m : r->group.members) m->have_volume = false;
    return fail(e, msg + " (device group: the upload failed on a member - no member keeps a volume)");
  }
  r->group.upload_ms = ms_since(t0);
  return 0;
}

int ovr_hip_get_upload_times(const ovr_hip_renderer* r, double out_ms[4])
{
  if (!r || !out_ms) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_upload_times: null argument");
  for (int i = 0; i < 4; ++i) out_ms[i] = r->upload_ms[i];
  if (r->group.members.size() > 1) out_ms[0] = r->group.upload_ms;
  return 0;
}

int ovr_hip_query_addressing_mode(const int32_t dims[3], int value_type, int32_t layout, int32_t n_colors, int32_t n_alphas)
{
  if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_query_addressing_mode: bad dims");
  const int vt = device_voxel_type(value_type);
  if (vt < 0) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_query_addressing_mode: unknown value type");
  const int rt = replica_voxel_type(vt, layout);
  if (layout < 0 || layout >= kLayouts || rt < 0) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_query_addressing_mode: the type has no such layout");
  VolumeDesc vd{};
  if (!volume_layout(rt, dims[0], dims[1], dims[2], vd)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_query_addressing_mode: the type has no such layout");
  if (!layout_offsets_fit(vd)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_query_addressing_mode: one z layer of this layout exceeds 2^32 elements - it is not built");
  return volume_addressing_mode(vd, n_colors, n_alphas);
}

} // extern "C"
