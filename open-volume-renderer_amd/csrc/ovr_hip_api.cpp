// ovr_hip_api.cpp - C ABI (include/ovr_hip.h) of the MI355X ray-marching backend: the extern "C" layer of the host-side state machine -
// create / destroy, the queued setters, commit diffing, render / sync, mapframe, swap and the getters.  The state machine itself lives in
// host/: state.hpp (the renderer's state), policy.hpp (the automatic decisions, free of HIP), commit_plan.hpp (what a changed parameter invalidates, free of
// HIP), ray_query.hpp (the known-answer ray queries as a table, free of HIP), buffers.cpp, volume.cpp, frame.cpp, group.cpp.
//
// Mirrors the host half of the reference's GPU device (citations relative to the reference tree):
//   queued setters + commit diffing ... ovr/renderer.h:135-285, ovr/devices/optix7/device_impl.cpp:113-197
//   render / frame_index / reset ...... device_impl.cpp:199-269
//   double-buffered framebuffer ....... ovr/devices/optix7/optix7_common.h:328-414, device_impl.cpp:102-111,271-281
// No CPU fallback exists: every entry point needs a HIP device and fails with OVR_HIP_EDEVICE otherwise.
#include "host/ray_query.hpp"
#include "host/state.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>

using namespace ovrhip;
using namespace ovrhip::host;

// a setter on a device group queues its value on every member (see GroupState::mtx)
#define GROUP_FORWARD(r, call)                                                                                          \
  do {                                                                                                                  \
    for (size_t i_ = 1; i_ < (r)->group.members.size(); ++i_) {                                                         \
      ovr_hip_renderer* m = (r)->group.members[i_];                                                                     \
      if (int e_ = (call)) { (void)hipSetDevice((r)->device); return e_; }                                              \
    }                                                                                                                   \
    if ((r)->group.members.size() > 1) (void)hipSetDevice((r)->device);                                                 \
  } while (0)

extern "C" {

const char* ovr_hip_last_error(void) { return g_last_error.c_str(); }
int ovr_hip_abi_version(void) { return OVR_HIP_ABI_VERSION; }

int ovr_hip_create(ovr_hip_renderer** out, int device_id)
{
  if (!out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_create: null output pointer");
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(OVR_HIP_EDEVICE, "[hip] no HIP device available - this backend has no CPU fallback");
  if (device_id < 0 || device_id >= count) return fail(OVR_HIP_EINVAL, "[hip] invalid device ordinal " + std::to_string(device_id));
  HIP_TRY(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return fail(OVR_HIP_EDEVICE, std::string("[hip] device is ") + prop.gcnArchName + ", this library is built for gfx950 (MI355X) only");
  ovr_hip_renderer* r = new ovr_hip_renderer();
  r->device = device_id;
  apply_lighting(r);
  apply_clip_box(r);
  auto acquire = [&]() -> int {
    HIP_TRY(hipStreamCreate(&r->own_stream[0]));
    HIP_TRY(hipStreamCreate(&r->own_stream[1]));
    for (int i = 0; i < 4; ++i) HIP_TRY(hipEventCreate(&r->ev[i]));
    {
      // replicas are built at the highest stream priority: the sooner a replica is resident, the sooner the frames that asked for it get faster
      int lo = 0, hi = 0;
      if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
      HIP_TRY(hipStreamCreateWithPriority(&r->build_stream, hipStreamNonBlocking, hi));
    }
    for (int k = 0; k < kLayouts; ++k) HIP_TRY(hipEventCreateWithFlags(&r->build_ev[k], hipEventDisableTiming));
    HIP_TRY(hipMalloc((void**)&r->d_counters, kFrameWordsBytes));
    HIP_TRY(hipMemset(r->d_counters, 0, kFrameWordsBytes));
    HIP_TRY(hipMalloc((void**)&r->d_sparse_count, sizeof(unsigned long long)));
    HIP_TRY(hipMalloc((void**)&r->d_data_range, minmax_reduce_floats() * sizeof(float)));
    // pinned, read by the host after a frame: 8 counters, then the pool's control words (written by the frame's last reduction kernel)
    HIP_TRY(hipHostMalloc((void**)&r->h_counters, 8 * sizeof(unsigned long long) + (size_t)kPoolCtrlWords * sizeof(unsigned int), hipHostMallocDefault));
    r->h_ctrl = reinterpret_cast<unsigned int*>(r->h_counters + 8);
    return 0;
  };
  if (int e = acquire()) { ovr_hip_destroy(r); return e; } // nothing half-built leaks
  std::memset(r->h_counters, 0, 8 * sizeof(unsigned long long) + (size_t)kPoolCtrlWords * sizeof(unsigned int));
  // defaults of the reference's parameter block (params.h:55-99, renderer.h:255-285)
  r->spp.init(1);
  r->sparse.init(0);
  r->accumulate.init(0);
  r->shading.init(OVR_HIP_SHADE_FULL);
  r->grid_convention.init(OVR_HIP_GRID_CELL_CENTRED);
  r->rate.init(1.f);
  r->layouts.init(1);
  r->layout_choice.init(-1);
  if (const char* f = getenv("OVR_HIP_LAYOUTS")) r->layouts.init(atoi(f)); // diagnostic override
  if (const char* f = getenv("OVR_HIP_SKIP_ADAPTIVE")) r->skip.adaptive = atoi(f) != 0;
  if (const char* f = getenv("OVR_HIP_TUNE")) r->tune.on = atoi(f) != 0;
  if (const char* f = getenv("OVR_HIP_SHADE_ORDER")) r->shade_order_on = atoi(f) != 0;
  if (const char* f = getenv("OVR_HIP_ROW_LOADS")) r->P.row_loads = atoi(f) != 0 ? 2 : 1; // (RayMarchParams::row_loads; 0 = by size)
  if (const char* f = getenv("OVR_HIP_SHADE_BEAM")) r->shade_beam = std::max(1.f, (float)atof(f));
  *out = r;
  return 0;
}
void ovr_hip_destroy(ovr_hip_renderer* r)
{
  if (!r) return;
  if (r->group.members.size() > 1) group_stop_workers(r);
  for (size_t i = 1; i < r->group.members.size(); ++i) ovr_hip_destroy(r->group.members[i]); // a group leader takes its followers with it
  r->group.members.clear();
  join_builders(r);
  (void)hipSetDevice(r->device);
  (void)hipDeviceSynchronize();
  group_release(r);
  (void)free_framebuffers(r);
  for (int k = 0; k < kLayouts; ++k) {
    if (r->d_replica[k]) (void)hipFree(r->d_replica[k]);
    if (r->d_axis[k]) (void)hipFree(r->d_axis[k]);
  }
  if (r->d_tf_color) (void)hipFree(r->d_tf_color);
  if (r->h_tf) (void)hipHostFree(r->h_tf);
  if (r->ev_tf) (void)hipEventDestroy(r->ev_tf);
  if (r->d_noise) (void)hipFree(r->d_noise);
  if (r->d_mc_minmax) (void)hipFree(r->d_mc_minmax);
  if (r->d_ao_dirs) (void)hipFree(r->d_ao_dirs);
  if (r->d_preint_nodes) (void)hipFree(r->d_preint_nodes);
  if (r->d_max_depth) (void)hipFree(r->d_max_depth);
  if (r->d_max_depth_queued) (void)hipFree(r->d_max_depth_queued);
  if (r->d_mc_majorant) (void)hipFree(r->d_mc_majorant);
  if (r->d_mc_occupancy) (void)hipFree(r->d_mc_occupancy);
  if (r->d_mc_fine) (void)hipFree(r->d_mc_fine);
  if (r->d_counters) (void)hipFree(r->d_counters);
  if (r->d_sparse_count) (void)hipFree(r->d_sparse_count);
  if (r->d_data_range) (void)hipFree(r->d_data_range);
  if (r->d_update_stage) (void)hipFree(r->d_update_stage);
  free_shadow_cache(r);
  if (r->h_counters) (void)hipHostFree(r->h_counters);
  if (r->conv.h_publish) (void)hipHostFree(r->conv.h_publish);
  if (r->recon.h_publish) (void)hipHostFree(r->recon.h_publish);
  for (int i = 0; i < 2; ++i) if (r->recon.ev[i]) (void)hipEventDestroy(r->recon.ev[i]);
  for (int i = 0; i < 4; ++i) if (r->ev[i]) (void)hipEventDestroy(r->ev[i]);
  if (r->pool.reqs) (void)hipFree(r->pool.reqs);
  if (r->pool.chunk_next) (void)hipFree(r->pool.chunk_next);
  if (r->pool.chunk_n) (void)hipFree(r->pool.chunk_n);
  if (r->pool.shade_counters) (void)hipFree(r->pool.shade_counters);
  if (r->pool.order) (void)hipFree(r->pool.order);
  if (r->pool.order_key) (void)hipFree(r->pool.order_key);
  if (r->pool.order_ws) (void)hipFree(r->pool.order_ws);

  if (r->d_block_counters) (void)hipFree(r->d_block_counters);
  if (r->sched.h_info) (void)hipHostFree(r->sched.h_info);
  if (r->d_trace) (void)hipFree(r->d_trace);
  for (int i = 0; i < 2; ++i)
    if (r->own_stream[i]) (void)hipStreamDestroy(r->own_stream[i]);
  if (r->build_stream) (void)hipStreamDestroy(r->build_stream);
  for (int k = 0; k < kLayouts; ++k)
    if (r->build_ev[k]) (void)hipEventDestroy(r->build_ev[k]);
  delete r;
}

int ovr_hip_set_stream(ovr_hip_renderer* r, void* s)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (r->group.members.size() > 1 && s) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_stream: a device group renders on one stream per device");
  if (int e = finish_frame(r)) return e;
  HIP_TRY(hipStreamSynchronize(r->stream())); // table copies and the like enqueued on the stream that is being left
  // ... and what a reset left on the OTHER set's own stream (its memsets: enqueue_frame; a table copy recorded there): the caller's stream is not
  // ordered behind either of them
  for (int i = 0; i < 2; ++i) HIP_TRY(hipStreamSynchronize(r->own_stream[i]));
  r->user_stream = (hipStream_t)s;
  r->use_user_stream = (s != nullptr);
  return 0;
}
int ovr_hip_set_phase_timing(ovr_hip_renderer* r, int32_t on)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  GroupLock gl(r);
  r->phase_timing.store(on != 0); // read when the next frame is launched; a frame in flight keeps what it was launched with
  GROUP_FORWARD(r, ovr_hip_set_phase_timing(m, on));
  return 0;
}

int ovr_hip_set_grid_convention(ovr_hip_renderer* r, int c)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (c != OVR_HIP_GRID_CELL_CENTRED && c != OVR_HIP_GRID_VERTEX_CENTRED) return fail(OVR_HIP_EINVAL, "[hip] unknown grid convention");
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->grid_convention.set(c); }
  GROUP_FORWARD(r, ovr_hip_set_grid_convention(m, c));
  return 0;
}

int ovr_hip_set_transfer_function(ovr_hip_renderer* r, const float* colors, int32_t n_colors, const float* alphas, int32_t n_alphas,
                                  float lo, float hi)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (n_colors < 0 || n_alphas < 0 || (n_colors > 0 && !colors) || (n_alphas > 0 && !alphas))
    return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_transfer_function: bad arguments");
  GroupLock gl(r);
  {
    std::lock_guard<std::mutex> lk(r->mtx);
    TfnP t;
    t.colors.assign(colors, colors + (size_t)n_colors * 3);
    t.alphas.assign(alphas, alphas + (size_t)n_alphas * 2);
    t.lo = lo;
    t.hi = hi;
    r->tfn.set(t);
  }
  GROUP_FORWARD(r, ovr_hip_set_transfer_function(m, colors, n_colors, alphas, n_alphas, lo, hi));
  return 0;
}

int ovr_hip_set_camera(ovr_hip_renderer* r, const float from[3], const float at[3], const float up[3], float fovy)
{
  if (!r || !from || !at || !up) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_camera: null argument");
  GroupLock gl(r);
  {
    std::lock_guard<std::mutex> lk(r->mtx);
    CameraP c;
    std::memcpy(c.from, from, sizeof(c.from));
    std::memcpy(c.at, at, sizeof(c.at));
    std::memcpy(c.up, up, sizeof(c.up));
    c.fovy = fovy;
    r->camera.set(c);
  }
  GROUP_FORWARD(r, ovr_hip_set_camera(m, from, at, up, fovy));
  return 0;
}

int ovr_hip_set_camera_orthographic(ovr_hip_renderer* r, const float from[3], const float at[3], const float up[3], float height)
{
  if (!r || !from || !at || !up) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_camera_orthographic: null argument");
  if (!std::isfinite(height) || !(height > 0.f)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_camera_orthographic: the height must be finite and > 0");
  GroupLock gl(r);
  {
    std::lock_guard<std::mutex> lk(r->mtx);
    CameraP c;
    std::memcpy(c.from, from, sizeof(c.from));
    std::memcpy(c.at, at, sizeof(c.at));
    std::memcpy(c.up, up, sizeof(c.up));
    c.fovy = 0.f;
    c.kind = OVR_HIP_CAMERA_ORTHOGRAPHIC;
    c.height = height;
    r->camera.set(c); // the perspective camera's slot: recorded under the commit plan's kCamera
  }
  GROUP_FORWARD(r, ovr_hip_set_camera_orthographic(m, from, at, up, height));
  return 0;
}

int ovr_hip_get_camera(const ovr_hip_renderer* r, ovr_hip_camera* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_camera: null argument");
  std::lock_guard<std::mutex> lk(const_cast<ovr_hip_renderer*>(r)->mtx);
  const CameraP& c = r->camera.current;
  const RayMarchParams& P = r->P;
  std::memset(out, 0, sizeof(*out));
  out->kind = c.kind;
  std::memcpy(out->from, c.from, sizeof(c.from));
  std::memcpy(out->at, c.at, sizeof(c.at));
  std::memcpy(out->up, c.up, sizeof(c.up));
  out->fovy = c.kind == OVR_HIP_CAMERA_ORTHOGRAPHIC ? 0.f : c.fovy;
  out->height = c.kind == OVR_HIP_CAMERA_ORTHOGRAPHIC ? c.height : 0.f;
  if (!r->camera_dirty) { // (dirty: no framebuffer size was committed yet, update_camera has not run for this camera)
    out->pos[0] = P.cam_pos.x; out->pos[1] = P.cam_pos.y; out->pos[2] = P.cam_pos.z;
    out->dir[0] = P.cam_dir.x; out->dir[1] = P.cam_dir.y; out->dir[2] = P.cam_dir.z;
    out->hor[0] = P.cam_hor.x; out->hor[1] = P.cam_hor.y; out->hor[2] = P.cam_hor.z;
    out->ver[0] = P.cam_ver.x; out->ver[1] = P.cam_ver.y; out->ver[2] = P.cam_ver.z;
  }
  return 0;
}

int ovr_hip_set_fbsize(ovr_hip_renderer* r, int32_t w, int32_t h)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (w < 0 || h < 0) return fail(OVR_HIP_EINVAL, "[hip] negative framebuffer size");
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); Size2 s; s.w = w; s.h = h; r->fbsize.set(s); }
  GROUP_FORWARD(r, ovr_hip_set_fbsize(m, w, h));
  return 0;
}

#define OVR_SIMPLE_SETTER(name, field, type, check, msg)                                                               \
  int name(ovr_hip_renderer* r, type v)                                                                                \
  {                                                                                                                    \
    if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");                                                        \
    if (!(check)) return fail(OVR_HIP_EINVAL, msg);                                                                    \
    GroupLock gl(r);                                                                                                   \
    { std::lock_guard<std::mutex> lk(r->mtx); r->field.set(v); }                                                       \
    GROUP_FORWARD(r, name(m, v));                                                                                      \
    return 0;                                                                                                          \
  }
OVR_SIMPLE_SETTER(ovr_hip_set_sample_per_pixel, spp, int32_t, v > 0, "'sample_per_pixel' should always be positive")
OVR_SIMPLE_SETTER(ovr_hip_set_volume_sampling_rate, rate, float, v > 0.f, "[hip] sampling rate must be positive")
OVR_SIMPLE_SETTER(ovr_hip_set_frame_accumulation, accumulate, int32_t, true, "")
OVR_SIMPLE_SETTER(ovr_hip_set_sparse_sampling, sparse, int32_t, true, "")
OVR_SIMPLE_SETTER(ovr_hip_set_shading, shading, int32_t, v >= 0 && v <= 2, "[hip] unknown shading mode")
OVR_SIMPLE_SETTER(ovr_hip_set_projection, projection, int32_t, v >= OVR_HIP_PROJECT_OFF && v <= OVR_HIP_PROJECT_MEAN, "[hip] ovr_hip_set_projection: unknown mode")
OVR_SIMPLE_SETTER(ovr_hip_set_shading_pipeline, pipeline, int32_t, v >= 0 && v <= 2, "[hip] unknown shading pipeline")
OVR_SIMPLE_SETTER(ovr_hip_set_empty_space_skipping, skipping, int32_t, true, "")
OVR_SIMPLE_SETTER(ovr_hip_set_volume_layouts, layouts, int32_t, v >= 0 && v <= 2, "[hip] unknown volume-layout mode")
OVR_SIMPLE_SETTER(ovr_hip_set_layout_choice, layout_choice, int32_t, v >= -1 && v < kLayouts, "[hip] unknown layout choice")
OVR_SIMPLE_SETTER(ovr_hip_set_lds_staging, lds_staging, int32_t, v == 0 || v == 1, "[hip] unknown LDS-staging mode")
OVR_SIMPLE_SETTER(ovr_hip_set_pixel_jitter, jitter, int32_t, v == 0 || v == 1, "[hip] unknown pixel-jitter mode")

int ovr_hip_get_projection(const ovr_hip_renderer* r, ovr_hip_projection* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_projection: null argument");
  out->mode = r->projection.current;
  out->range_skipping = r->projection_skipped ? 1 : 0;
  return 0;
}

// both setters of the isosurfaces: one queued slot.  opacities == nullptr: all 1, the opaque level sets
int ovr_hip_set_isosurface_layers(ovr_hip_renderer* r, const float* isovalues, const float* opacities, int32_t n)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (n < 0 || n > OVR_HIP_MAX_ISOVALUES || (n > 0 && !isovalues)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_isosurfaces: between 0 and 4 isovalues");
  IsoP p;
  p.n = n;
  int order[OVR_HIP_MAX_ISOVALUES] = { 0, 1, 2, 3 };
  for (int k = 0; k < n; ++k) {
    if (!std::isfinite(isovalues[k])) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_isosurfaces: the isovalues must be finite");
    if (opacities && !(std::isfinite(opacities[k]) && opacities[k] > 0.f && opacities[k] <= 1.f))
      return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_isosurface_layers: an opacity lies in (0, 1]");
  }
  std::sort(order, order + n, [&](int a, int b) { return isovalues[a] < isovalues[b]; });
  for (int k = 0; k < n; ++k) { // the opacities travel with their isovalues
    p.v[k] = isovalues[order[k]];
    p.a[k] = opacities ? opacities[order[k]] : 1.f;
  }
  for (int k = 1; k < n; ++k)
    if (p.v[k] == p.v[k - 1]) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_isosurfaces: two isovalues are equal");
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->isosurfaces.set(p); }
  GROUP_FORWARD(r, ovr_hip_set_isosurface_layers(m, isovalues, opacities, n));
  return 0;
}

int ovr_hip_set_isosurfaces(ovr_hip_renderer* r, const float* isovalues, int32_t n) { return ovr_hip_set_isosurface_layers(r, isovalues, nullptr, n); }

int ovr_hip_get_isosurface_layers(const ovr_hip_renderer* r, ovr_hip_isosurface_layers* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_isosurface_layers: null argument");
  const IsoP& p = r->isosurfaces.current;
  out->n = p.n;
  for (int k = 0; k < OVR_HIP_MAX_ISOVALUES; ++k) {
    out->isovalues[k] = k < p.n ? p.v[k] : 0.f;
    out->opacities[k] = k < p.n ? p.a[k] : 0.f;
  }
  out->translucent = p.translucent() ? 1 : 0;
  out->range_skipping = r->isosurface_skipped ? 1 : 0;
  return 0;
}

int ovr_hip_get_isosurfaces(const ovr_hip_renderer* r, ovr_hip_isosurfaces* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_isosurfaces: null argument");
  const IsoP& p = r->isosurfaces.current;
  out->n = p.n;
  for (int k = 0; k < OVR_HIP_MAX_ISOVALUES; ++k) out->isovalues[k] = k < p.n ? p.v[k] : 0.f;
  out->range_skipping = r->isosurface_skipped ? 1 : 0;
  return 0;
}

int ovr_hip_set_slices(ovr_hip_renderer* r, const ovr_hip_slice* slices, int32_t n)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (n < 0 || n > OVR_HIP_MAX_SLICES) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_slices: between 0 and 4 slices");
  if (!slices && n > 0) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_slices: a null pointer with n > 0");
  SliceP p;
  p.n = n;
  for (int k = 0; k < n; ++k) {
    SliceValues v;
    if (const char* why = slice_values(slices[k].point, slices[k].normal, slices[k].thickness, slices[k].mode, &v))
      return fail(OVR_HIP_EINVAL, std::string("[hip] ovr_hip_set_slices: ") + why);
    for (int a = 0; a < 3; ++a) p.normal[k][a] = v.normal[a];
    p.c[k] = v.c;
    p.thickness[k] = slices[k].thickness;
    p.mode[k] = slices[k].mode;
  }
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->slices.set(p); }
  GROUP_FORWARD(r, ovr_hip_set_slices(m, slices, n));
  return 0;
}

int ovr_hip_get_slices(const ovr_hip_renderer* r, ovr_hip_slices* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_slices: null argument");
  const SliceP& p = r->slices.current;
  std::memset(out, 0, sizeof(*out));
  out->n = p.n;
  for (int k = 0; k < p.n; ++k) {
    for (int a = 0; a < 3; ++a) out->slice[k].normal[a] = p.normal[k][a];
    out->slice[k].c = p.c[k];
    out->slice[k].thickness = p.thickness[k];
    out->slice[k].mode = p.mode[k];
  }
  out->walks = p.walks() ? 1 : 0;
  out->range_skipping = r->slices_skipped ? 1 : 0;
  return 0;
}

int ovr_hip_set_slice_context(ovr_hip_renderer* r, int32_t mode, float opacity_scale)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (mode != OVR_HIP_SLICE_CONTEXT_OFF && mode != OVR_HIP_SLICE_CONTEXT_FRONT) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_slice_context: the mode is OFF or FRONT");
  SliceContextP p;
  p.mode = mode;
  if (mode != OVR_HIP_SLICE_CONTEXT_OFF) { // (ignored, and stored as 1, in mode OFF)
    if (!(opacity_scale >= 0.f && opacity_scale <= 1.f)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_slice_context: the opacity scale lies in [0, 1]");
    p.scale = opacity_scale;
  }
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->slice_context.set(p); }
  GROUP_FORWARD(r, ovr_hip_set_slice_context(m, mode, opacity_scale));
  return 0;
}

int ovr_hip_get_slice_context(const ovr_hip_renderer* r, ovr_hip_slice_context* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_slice_context: null argument");
  const SliceContextP& p = r->slice_context.current;
  std::memset(out, 0, sizeof(*out));
  out->mode = p.mode;
  out->opacity_scale = p.scale;
  out->active = (p.mode == OVR_HIP_SLICE_CONTEXT_FRONT && committed_frame(r) == CommittedFrame::Slices) ? 1 : 0;
  return 0;
}

int ovr_hip_set_isosurface_context(ovr_hip_renderer* r, int32_t mode, float opacity_scale)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (mode != OVR_HIP_ISO_CONTEXT_OFF && mode != OVR_HIP_ISO_CONTEXT_VOLUME) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_isosurface_context: the mode is OFF or VOLUME");
  IsoContextP p;
  p.mode = mode;
  if (mode != OVR_HIP_ISO_CONTEXT_OFF) { // (ignored, and stored as 1, in mode OFF)
    if (!(opacity_scale >= 0.f && opacity_scale <= 1.f)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_isosurface_context: the opacity scale lies in [0, 1]");
    p.scale = opacity_scale;
  }
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->isosurface_context.set(p); }
  GROUP_FORWARD(r, ovr_hip_set_isosurface_context(m, mode, opacity_scale));
  return 0;
}

int ovr_hip_get_isosurface_context(const ovr_hip_renderer* r, ovr_hip_isosurface_context* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_isosurface_context: null argument");
  const IsoContextP& p = r->isosurface_context.current;
  std::memset(out, 0, sizeof(*out));
  out->mode = p.mode;
  out->opacity_scale = p.scale;
  out->active = (p.mode == OVR_HIP_ISO_CONTEXT_VOLUME && committed_frame(r) == CommittedFrame::Isovalues) ? 1 : 0;
  return 0;
}

int ovr_hip_set_preintegration(ovr_hip_renderer* r, int32_t mode)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (mode != OVR_HIP_PREINTEGRATION_OFF && mode != OVR_HIP_PREINTEGRATION_SEGMENTS) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_preintegration: the mode is OFF or SEGMENTS");
  PreintP p;
  p.mode = mode;
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->preintegration.set(p); }
  GROUP_FORWARD(r, ovr_hip_set_preintegration(m, mode));
  return 0;
}

int ovr_hip_get_preintegration(const ovr_hip_renderer* r, ovr_hip_preintegration* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_preintegration: null argument");
  std::memset(out, 0, sizeof(*out));
  out->mode = r->preintegration.current.mode;
  out->active = preintegrated_frame(r) ? 1 : 0;
  // (the table of the last pre-integrated frame or tables getter: 0 until one was built, and while a newer transfer function awaits its rebuild)
  const bool fresh = r->preint_nodes > 0 && r->preint_generation == r->tf_generation;
  out->nodes = fresh ? r->preint_nodes : 0;
  out->subdivision = fresh ? r->preint_subdivision : 0;
  return 0;
}

int ovr_hip_get_preintegration_tables(ovr_hip_renderer* r, float* nodes_host, size_t capacity_nodes, int32_t* n_nodes)
{
  if (!r || !n_nodes) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_preintegration_tables: null argument");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  if (!r->have_volume) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_preintegration_tables: no volume was set");
  if (!r->d_tf_color || !r->d_tf_alpha || !r->h_tf) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_preintegration_tables: no transfer function was committed");
  // the table a pre-integrated frame of the committed volume, transfer function and clip box would read, whatever mode and shading are committed
  RayMarchParams q = r->P;
  fill_shadow_params(r, q);
  q.shading = 0; q.projection = 0; q.iso_n = 0; q.slice_n = 0; q.ao_samples = 0;
  q.pool = PoolDesc{}; q.majorant = nullptr; q.sparse_xy = nullptr; q.schedule = nullptr; q.n_schedule = 0;
  if (int e = bind_preintegration(r, q)) return e;
  if (!q.preint_nodes) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_preintegration_tables: the node table does not fit the frame's LDS budget beside this transfer function");
  *n_nodes = r->preint_nodes;
  if (nodes_host) {
    if (capacity_nodes < (size_t)r->preint_nodes) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_preintegration_tables: nodes_host holds fewer than n_nodes nodes");
    std::memcpy(nodes_host, r->preint_table.data(), (size_t)r->preint_nodes * 4 * sizeof(float));
  }
  return 0;
}

static_assert(kGradientOpacityOff == OVR_HIP_GRADIENT_OPACITY_OFF && kGradientOpacityRamp == OVR_HIP_GRADIENT_OPACITY_RAMP, "host/gradient_opacity_host.hpp restates include/ovr_hip.h");
int ovr_hip_set_gradient_opacity(ovr_hip_renderer* r, int32_t mode, float lo, float hi)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  GradientOpacityState g;
  if (!gradient_opacity_commit(mode, lo, hi, &g))
    return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_gradient_opacity: the mode is OFF or RAMP, the thresholds are finite and lo < hi");
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->gradient_opacity.set(g); }
  GROUP_FORWARD(r, ovr_hip_set_gradient_opacity(m, mode, lo, hi));
  return 0;
}

int ovr_hip_get_gradient_opacity(const ovr_hip_renderer* r, ovr_hip_gradient_opacity* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_gradient_opacity: null argument");
  std::memset(out, 0, sizeof(*out));
  const GradientOpacityState& g = r->gradient_opacity.current;
  out->mode = g.mode;
  out->active = gradient_opacity_frame(r) ? 1 : 0;
  out->lo = g.lo;
  out->hi = g.hi;
  out->inv_ramp = g.inv_ramp;
  return 0;
}

} // extern "C"
namespace {
// one renderer's copy of the caller's image, from host memory (null: the limit is switched off), into the QUEUED buffer, which only ever grows.  The frame in
// flight is resolved first, as ovr_hip_set_volume does: after a commit has swapped the buffers the queued one is the image an earlier frame was drawn from, and
// no frame may see it half written.  The copy is synchronous: `host` is not referenced after the call returns
int set_max_depth_one(ovr_hip_renderer* r, const float* host, int width, int height)
{
  MaxDepthState m;
  if (host) {
    if (int e = set_device(r)) return e;
    if (int e = finish_frame_one(r)) return e;
    const size_t n = (size_t)width * (size_t)height;
    if (r->max_depth_queued_capacity < n) {
      float* d = nullptr;
      if (hipMalloc((void**)&d, n * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OVR_HIP_EDEVICE, "[hip] ovr_hip_set_max_depth: the image of " + std::to_string(n) + " pixels could not be allocated");
      }
      if (r->d_max_depth_queued) HIP_TRY(hipFree(r->d_max_depth_queued));
      r->d_max_depth_queued = d;
      r->max_depth_queued_capacity = n;
    }
    if (hipMemcpy(r->d_max_depth_queued, host, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      return fail(OVR_HIP_EDEVICE, "[hip] ovr_hip_set_max_depth: the copy to the device failed");
    }
    m.on = true; m.width = width; m.height = height;
  }
  std::lock_guard<std::mutex> lk(r->mtx);
  r->max_depth.set(m);
  return 0;
}
} // namespace
extern "C" {

int ovr_hip_set_max_depth(ovr_hip_renderer* r, const float* depth, int mem_kind, int32_t width, int32_t height)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (const int rule = max_depth_check(depth, mem_kind, width, height)) return fail(OVR_HIP_EINVAL, std::string("[hip] ovr_hip_set_max_depth: ") + max_depth_rule_text(rule));
  // validated once, on the handle the caller holds; every member of a device group then uploads the same host copy of the whole image
  std::vector<float> stage;
  const float* host = depth;
  if (depth && mem_kind == OVR_HIP_MEM_DEVICE) {
    if (int e = set_device(r)) return e;
    stage.resize((size_t)width * (size_t)height);
    HIP_TRY(hipMemcpy(stage.data(), depth, stage.size() * sizeof(float), hipMemcpyDeviceToHost));
    host = stage.data();
  }
  if (r->group.members.size() <= 1) return set_max_depth_one(r, host, width, height);
  if (int e = finish_frame(r)) return e;
  GroupLock gl(r);
  return group_call(r, [=](ovr_hip_renderer* m) { return set_max_depth_one(m, host, width, height); }, [&] { return set_max_depth_one(r, host, width, height); });
}

int ovr_hip_get_max_depth(const ovr_hip_renderer* r, ovr_hip_max_depth* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_max_depth: null argument");
  std::memset(out, 0, sizeof(*out));
  const MaxDepthState& m = r->max_depth.current;
  out->mode = m.on ? OVR_HIP_MAX_DEPTH_ON : OVR_HIP_MAX_DEPTH_OFF;
  out->active = max_depth_frame(r) ? 1 : 0;
  out->width = m.on ? m.width : 0;
  out->height = m.on ? m.height : 0;
  return 0;
}

int ovr_hip_get_max_depth_values(ovr_hip_renderer* r, float* depth_host, size_t capacity_floats, int32_t* width, int32_t* height)
{
  if (!r || !width || !height) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_max_depth_values: null argument");
  const MaxDepthState& m = r->max_depth.current;
  *width = m.on ? m.width : 0;
  *height = m.on ? m.height : 0;
  if (!m.on || !depth_host) return 0;
  const size_t n = (size_t)m.width * (size_t)m.height;
  if (capacity_floats < n) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_max_depth_values: the buffer holds fewer than width x height floats");
  if (!r->d_max_depth || r->max_depth_capacity < n) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_max_depth_values: no image is resident");
  if (int e = set_device(r)) return e;
  HIP_TRY(hipMemcpy(depth_host, r->d_max_depth, n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

static_assert(kDepthOutputOff == OVR_HIP_DEPTH_OUTPUT_OFF && kDepthOutputOn == OVR_HIP_DEPTH_OUTPUT_ON, "host/depth_output_host.hpp restates include/ovr_hip.h");
int ovr_hip_set_depth_output(ovr_hip_renderer* r, int32_t mode, float threshold)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (const int rule = depth_output_check(mode, threshold)) return fail(OVR_HIP_EINVAL, std::string("[hip] ovr_hip_set_depth_output: ") + depth_output_rule_text(rule));
  DepthOutputState s;
  s.mode = mode;
  s.threshold = mode == kDepthOutputOn ? threshold : 0.f;
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->depth_output.set(s); }
  GROUP_FORWARD(r, ovr_hip_set_depth_output(m, mode, threshold));
  return 0;
}

int ovr_hip_get_depth_output(const ovr_hip_renderer* r, ovr_hip_depth_output* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_depth_output: null argument");
  std::memset(out, 0, sizeof(*out));
  const DepthOutputState& s = r->depth_output.current;
  out->mode = s.mode;
  out->active = depth_output_frame(r) ? 1 : 0;
  out->limited = depth_output_limited(depth_output_frame(r), true, max_depth_frame(r)) ? 1 : 0;
  out->threshold = s.threshold;
  return 0;
}

int ovr_hip_set_ambient_occlusion(ovr_hip_renderer* r, int32_t samples, float distance)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (samples < 0 || samples > OVR_HIP_MAX_AO_SAMPLES) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_ambient_occlusion: between 0 and 16 samples");
  if (samples > 0 && !(distance > 0.f)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_ambient_occlusion: the distance must be positive (+inf: the whole box)");
  AoP p;
  p.samples = samples;
  p.distance = samples > 0 ? distance : INFINITY; // (not read while K == 0)
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->ambient_occlusion.set(p); }
  GROUP_FORWARD(r, ovr_hip_set_ambient_occlusion(m, samples, distance));
  return 0;
}

int ovr_hip_get_ambient_occlusion(const ovr_hip_renderer* r, ovr_hip_ambient_occlusion* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_ambient_occlusion: null argument");
  const AoP& p = r->ambient_occlusion.current;
  out->samples = p.samples;
  out->distance = p.distance;
  out->rotations = OVR_HIP_AO_ROTATIONS;
  // as include/ovr_hip.h defines it - of the next ISOSURFACE frame: committed slices and the isosurface context, under which no frame casts it, are not read
  out->active = p.samples > 0 && r->isosurfaces.current.n > 0 && r->shading.current != OVR_HIP_SHADE_NONE ? 1 : 0;
  return 0;
}

int ovr_hip_get_ambient_occlusion_directions(const ovr_hip_renderer* r, float* out, size_t capacity_floats)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_ambient_occlusion_directions: null argument");
  if (capacity_floats < r->ao_table.size()) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_ambient_occlusion_directions: the buffer holds fewer than 16 x K x 3 floats");
  std::copy(r->ao_table.begin(), r->ao_table.end(), out);
  return 0;
}

int ovr_hip_set_convergence(ovr_hip_renderer* r, int32_t mode, float threshold)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (mode != OVR_HIP_CONVERGENCE_OFF && mode != OVR_HIP_CONVERGENCE_ESTIMATE && mode != OVR_HIP_CONVERGENCE_ADAPTIVE)
    return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_convergence: unknown mode");
  if (!std::isfinite(threshold) || threshold < 0.f) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_convergence: the threshold must be finite and not negative");
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); ConvP c; c.mode = mode; c.threshold = threshold; r->convergence.set(c); }
  GROUP_FORWARD(r, ovr_hip_set_convergence(m, mode, threshold));
  return 0;
}

int ovr_hip_set_light(ovr_hip_renderer* r, const float direction[3], float intensity)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  LightP l; // the reference's literal
  if (direction) {
    const float len2 = direction[0] * direction[0] + direction[1] * direction[1] + direction[2] * direction[2];
    if (!std::isfinite(direction[0]) || !std::isfinite(direction[1]) || !std::isfinite(direction[2]) || !std::isfinite(len2) || !(len2 > 0.f)
        || !std::isfinite(1.f / std::sqrt(len2)))
      return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_light: the direction must be finite and have a length a float can normalise");
    std::memcpy(l.dir, direction, sizeof(l.dir));
  }
  if (!std::isfinite(intensity) || intensity < 0.f) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_light: the intensity must be finite and not negative");
  l.intensity = intensity;
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->light.set(l); }
  GROUP_FORWARD(r, ovr_hip_set_light(m, direction, intensity));
  return 0;
}

int ovr_hip_set_material(ovr_hip_renderer* r, float ambient, float diffuse, float specular, float shininess)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  for (float v : { ambient, diffuse, specular, shininess })
    if (!std::isfinite(v) || v < 0.f) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_material: every value must be finite and not negative");
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); MaterialP p; p.ambient = ambient; p.diffuse = diffuse; p.specular = specular; p.shininess = shininess; r->material.set(p); }
  GROUP_FORWARD(r, ovr_hip_set_material(m, ambient, diffuse, specular, shininess));
  return 0;
}

int ovr_hip_get_lighting(const ovr_hip_renderer* r, ovr_hip_lighting* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_lighting: null argument");
  const RayMarchParams& P = r->P;
  out->direction[0] = P.light.x; out->direction[1] = P.light.y; out->direction[2] = P.light.z;
  out->intensity = r->light.current.intensity;
  out->ambient = P.mat_ka; out->diffuse = P.mat_kd; out->specular = P.mat_ks; out->shininess = P.mat_shininess;
  const LightP lit;
  const MaterialP ref;
  out->is_reference = std::memcmp(r->light.current.dir, lit.dir, sizeof(lit.dir)) == 0 && r->light.current.intensity == 1.f && P.mat_ka == ref.ambient
                      && P.mat_kd == ref.diffuse && P.mat_ks == 0.f;
  return 0;
}

int ovr_hip_set_clip_box(ovr_hip_renderer* r, const float lower[3], const float upper[3])
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if ((lower == nullptr) != (upper == nullptr)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_clip_box: lower and upper must both be given, or both be NULL (no clip box)");
  ClipP c; // none
  if (lower) {
    for (int k = 0; k < 3; ++k)
      if (std::isnan(lower[k]) || std::isnan(upper[k]) || lower[k] > upper[k])
        return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_clip_box: the bounds must not be NaN, and lower must not exceed upper");
    c.enabled = 1;
    std::memcpy(c.lower, lower, sizeof(c.lower));
    std::memcpy(c.upper, upper, sizeof(c.upper));
  }
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->clip.set(c); }
  GROUP_FORWARD(r, ovr_hip_set_clip_box(m, lower, upper));
  return 0;
}

int ovr_hip_get_clip_box(const ovr_hip_renderer* r, ovr_hip_clip_box* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_clip_box: null argument");
  const RayMarchParams& P = r->P;
  const ClipP& c = r->clip.current;
  out->enabled = c.enabled;
  std::memcpy(out->lower, c.lower, sizeof(c.lower));
  std::memcpy(out->upper, c.upper, sizeof(c.upper));
  out->object_lower[0] = P.clip_lo.x; out->object_lower[1] = P.clip_lo.y; out->object_lower[2] = P.clip_lo.z;
  out->object_upper[0] = P.clip_hi.x; out->object_upper[1] = P.clip_hi.y; out->object_upper[2] = P.clip_hi.z;
  return 0;
}

int ovr_hip_set_shadow_cache(ovr_hip_renderer* r, int32_t mode, int32_t cell_voxels)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (mode != OVR_HIP_SHADOWS_MARCHED && mode != OVR_HIP_SHADOWS_CACHED && mode != OVR_HIP_SHADOWS_SUPPLIED)
    return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_shadow_cache: unknown mode");
  if (cell_voxels < 0) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_shadow_cache: the cell size must be at least 1 voxel (0 = the default)");
  ShadowP p;
  p.mode = mode;
  p.cell = cell_voxels > 0 ? cell_voxels : policy::kShadowCacheDefaultCell;
  if (mode == OVR_HIP_SHADOWS_CACHED && r->have_volume) {
    int dims[3];
    if (shadow_lattice_dims(r, p.cell, dims)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_shadow_cache: a lattice of more than 2^31 - 1 nodes (take a larger cell)");
  }
  if (mode == OVR_HIP_SHADOWS_SUPPLIED && !r->shadow_cache.d_supplied)
    return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_set_shadow_cache: mode SUPPLIED needs values first (ovr_hip_set_shadow_cache_values)");
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); r->shadow.set(p); }
  GROUP_FORWARD(r, ovr_hip_set_shadow_cache(m, mode, cell_voxels));
  return 0;
}

} // extern "C"
namespace {
// one renderer's copy of the caller's lattice, from host memory: the new buffer first, so that a failed allocation leaves the previous values in place
int set_shadow_values_one(ovr_hip_renderer* r, const float* host, const int32_t dims[3])
{
  if (int e = set_device(r)) return e;
  if (int e = finish_frame_one(r)) return e;
  const size_t nodes = (size_t)dims[0] * dims[1] * dims[2];
  float* d = nullptr;
  if (hipMalloc((void**)&d, nodes * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(OVR_HIP_EDEVICE, "[hip] ovr_hip_set_shadow_cache_values: the lattice of " + std::to_string(nodes) + " nodes could not be allocated");
  }
  if (hipMemcpy(d, host, nodes * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(d);
    return fail(OVR_HIP_EDEVICE, "[hip] ovr_hip_set_shadow_cache_values: the copy to the device failed");
  }
  HIP_TRY(hipDeviceSynchronize()); // no frame reads the old values any more
  ShadowCacheState& c = r->shadow_cache;
  if (c.d_supplied) HIP_TRY(hipFree(c.d_supplied));
  c.d_supplied = d;
  for (int k = 0; k < 3; ++k) c.supplied_dims[k] = dims[k];
  commit::Changes ch;
  ch.note(commit::kShadowValues, true, r->shadow.current.mode == OVR_HIP_SHADOWS_SUPPLIED);
  apply_effects(r, commit::plan_commit(ch, commit::CommitFacts()));
  return 0;
}
} // namespace
extern "C" {

int ovr_hip_set_shadow_cache_values(ovr_hip_renderer* r, const float* values, int mem_kind, const int32_t dims[3])
{
  if (!r || !values || !dims) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_shadow_cache_values: null argument");
  if (mem_kind != OVR_HIP_MEM_HOST && mem_kind != OVR_HIP_MEM_DEVICE) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_shadow_cache_values: bad mem_kind");
  long long nodes = 1;
  for (int k = 0; k < 3; ++k) {
    if (dims[k] < 2) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_shadow_cache_values: a lattice has at least 2 nodes per axis");
    nodes = nodes > 0x7fffffffll / dims[k] ? 0x80000000ll : nodes * dims[k];
  }
  if (nodes > 0x7fffffffll) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_shadow_cache_values: more than 2^31 - 1 nodes");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  // validated once, on the host, on the handle the caller holds; every member of a device group then uploads the same host copy
  std::vector<float> stage;
  const float* host = values;
  if (mem_kind == OVR_HIP_MEM_DEVICE) {
    stage.resize((size_t)nodes);
    HIP_TRY(hipMemcpy(stage.data(), values, (size_t)nodes * sizeof(float), hipMemcpyDeviceToHost));
    host = stage.data();
  }
  for (long long i = 0; i < nodes; ++i)
    if (!std::isfinite(host[i])) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_shadow_cache_values: value " + std::to_string(i) + " is not finite");
  const int32_t d3[3] = { dims[0], dims[1], dims[2] };
  if (r->group.members.size() <= 1) return set_shadow_values_one(r, host, d3);
  GroupLock gl(r);
  return group_call(r, [=](ovr_hip_renderer* m) { return set_shadow_values_one(m, host, d3); }, [&] { return set_shadow_values_one(r, host, d3); });
}

int ovr_hip_get_shadow_cache(const ovr_hip_renderer* r, ovr_hip_shadow_cache* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_shadow_cache: null argument");
  const ShadowCacheState& c = r->shadow_cache;
  const ShadowP& p = r->shadow.current;
  *out = ovr_hip_shadow_cache{};
  out->mode = p.mode;
  out->cell = p.cell;
  const int* dims = p.mode == OVR_HIP_SHADOWS_SUPPLIED ? c.supplied_dims : c.built_dims;
  const bool have = p.mode == OVR_HIP_SHADOWS_SUPPLIED ? c.d_supplied != nullptr : p.mode == OVR_HIP_SHADOWS_CACHED && c.d_built != nullptr && c.built_dims[0] > 0;
  if (have) {
    for (int k = 0; k < 3; ++k) out->dims[k] = dims[k];
    out->bytes = (uint64_t)dims[0] * dims[1] * dims[2] * sizeof(float);
    out->valid = p.mode == OVR_HIP_SHADOWS_SUPPLIED || c.built_valid ? 1 : 0;
  }
  out->builds = c.builds;
  out->build_shadow_samples = c.build_samples;
  out->build_ms = c.build_ms;
  return 0;
}

int ovr_hip_get_shadow_cache_values(ovr_hip_renderer* r, int32_t member, int32_t dims[3], float* values_host, float* positions_host, size_t capacity_nodes)
{
  if (!r || !dims) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_shadow_cache_values: null argument");
  const size_t members = std::max<size_t>(r->group.members.size(), 1);
  if (member < 0 || (size_t)member >= members) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_shadow_cache_values: no such member");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  ovr_hip_renderer* m = members > 1 ? r->group.members[(size_t)member] : r;
  if (m->shadow.current.mode == OVR_HIP_SHADOWS_MARCHED) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_shadow_cache_values: the committed mode is MARCHED - there is no lattice");
  auto read = [&]() -> int {
    if (int e = set_device(m)) return e;
    hipStream_t st = m->stream();
    RayMarchParams q = m->P;
    if (int e = ensure_shadow_cache(m, q, st)) return e;
    for (int k = 0; k < 3; ++k) dims[k] = q.shadow_n1[k] + 1;
    const size_t nodes = (size_t)dims[0] * dims[1] * dims[2];
    if (!values_host && !positions_host) return 0;
    if (capacity_nodes < nodes) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_shadow_cache_values: output too small");
    if (values_host) HIP_TRY(hipMemcpyAsync(values_host, q.shadow_lattice, nodes * sizeof(float), hipMemcpyDeviceToHost, st));
    if (positions_host) {
      if (!m->have_volume || !m->have_tfn) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_shadow_cache_values: the nodes' positions need a volume and a transfer function");
      float* d_pos = nullptr;
      HIP_TRY(hipMalloc((void**)&d_pos, nodes * 3 * sizeof(float)));
      const int d3[3] = { dims[0], dims[1], dims[2] };
      int e = shadow_lattice_positions(m, d3, d_pos, st);
      hipError_t err = e ? hipSuccess : hipMemcpyAsync(positions_host, d_pos, nodes * 3 * sizeof(float), hipMemcpyDeviceToHost, st);
      if (err == hipSuccess) err = hipStreamSynchronize(st);
      (void)hipFree(d_pos);
      if (e) return e;
      if (err != hipSuccess) return fail(OVR_HIP_EDEVICE, std::string("[hip] ovr_hip_get_shadow_cache_values: ") + hipGetErrorString(err));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  };
  const int e = read();
  (void)set_device(r);
  return e;
}

int ovr_hip_set_reconstruction(ovr_hip_renderer* r, int32_t mode)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (mode != OVR_HIP_RECONSTRUCT_OFF && mode != OVR_HIP_RECONSTRUCT_FILL) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_reconstruction: unknown mode");
  if (mode != OVR_HIP_RECONSTRUCT_OFF && (r->group.members.size() > 1 || r->group.leader))
    return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_set_reconstruction: a device group of more than one device does not reconstruct its frames - call "
                                "ovr_hip_reconstruct_image on the assembled frame");
  { std::lock_guard<std::mutex> lk(r->mtx); r->reconstruction.set(mode); }
  return 0;
}

int ovr_hip_set_focus(ovr_hip_renderer* r, float cx, float cy, float scale, float base_noise)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  GroupLock gl(r);
  { std::lock_guard<std::mutex> lk(r->mtx); FocusP f; f.cx = cx; f.cy = cy; f.scale = scale; f.base_noise = base_noise; r->focus.set(f); }
  GROUP_FORWARD(r, ovr_hip_set_focus(m, cx, cy, scale, base_noise));
  return 0;
}

int ovr_hip_set_noise_tile(ovr_hip_renderer* r, const float* tile, int32_t xy)
{
  if (!r || !tile || xy <= 0) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_noise_tile: bad arguments");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  HIP_TRY(hipDeviceSynchronize());
  if (r->d_noise) HIP_TRY(hipFree(r->d_noise));
  if (xy > 128) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_noise_tile: tiles larger than 128 x 128 are not supported");
  const size_t bytes = (size_t)xy * xy * 64 * sizeof(float);
  // stored transposed, [t][y][x], so that one frame's slice is contiguous (the reference's layout is [y][x][t])
  std::vector<float> tr((size_t)xy * xy * 64);
  for (int y = 0; y < xy; ++y)
    for (int x = 0; x < xy; ++x)
      for (int t = 0; t < 64; ++t) tr[((size_t)t * xy + y) * xy + x] = tile[((size_t)y * xy + x) * 64 + t];
  HIP_TRY(hipMalloc((void**)&r->d_noise, bytes));
  HIP_TRY(hipMemcpy(r->d_noise, tr.data(), bytes, hipMemcpyHostToDevice));
  r->noise_xy = xy;
  commit::Changes ch;
  ch.happened(commit::kNoiseTile);
  apply_effects(r, commit::plan_commit(ch, commit::CommitFacts()));
  if (r->group.members.size() > 1)
    if (int e = group_call(r, [=](ovr_hip_renderer* m) { return ovr_hip_set_noise_tile(m, tile, xy); })) return e;
  return 0;
}

int ovr_hip_set_image_shard(ovr_hip_renderer* r, int32_t rank, int32_t world, int32_t tw, int32_t th)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (world < 1 || rank < 0 || rank >= world || tw < 1 || th < 1) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_image_shard: bad arguments");
  GroupLock gl(r);
  if (r->group.members.size() > 1) { // a device group shards the image among its members itself: only the tile size is the caller's
    if (world != 1) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_set_image_shard: a device group cannot be one rank of a larger shard (use world = 1 to set its tile size)");
    for (size_t i = 0; i < r->group.members.size(); ++i) {
      ovr_hip_renderer* m = r->group.members[i];
      std::lock_guard<std::mutex> lk(m->mtx);
      ShardP s; s.rank = (int)i; s.world = (int)r->group.members.size(); s.tw = tw; s.th = th;
      m->shard.set(s);
    }
    return 0;
  }
  std::lock_guard<std::mutex> lk(r->mtx);
  ShardP s; s.rank = rank; s.world = world; s.tw = tw; s.th = th;
  r->shard.set(s);
  return 0;
}

} // extern "C"
namespace {
int commit_one(ovr_hip_renderer* r);
// what every member of a group must agree on after a commit (each applied its own copy of the queued values)
bool same_committed_state(const ovr_hip_renderer* a, const ovr_hip_renderer* b)
{
  auto same_bytes = [](const auto& x, const auto& y) { return std::memcmp(&x, &y, sizeof(x)) == 0; };
  // one comparison per forwarded parameter, in the order of commit_plan.hpp's table
  if (a->fbsize.current.w != b->fbsize.current.w || a->fbsize.current.h != b->fbsize.current.h) return false;
  if (!same_bytes(a->camera.current, b->camera.current)) return false;
  const TfnP &ta = a->tfn.current, &tb = b->tfn.current;
  if (!(ta.lo == tb.lo && ta.hi == tb.hi && ta.colors == tb.colors && ta.alphas == tb.alphas) || a->have_tfn != b->have_tfn) return false;
  if (a->grid_convention.current != b->grid_convention.current) return false;
  if (!same_bytes(a->focus.current, b->focus.current)) return false;
  if (a->spp.current != b->spp.current) return false;
  if (a->sparse.current != b->sparse.current) return false;
  if (a->accumulate.current != b->accumulate.current) return false;
  if (!(a->rate.current == b->rate.current)) return false;
  if (a->shading.current != b->shading.current || a->projection.current != b->projection.current) return false;
  if (!same_bytes(a->isosurfaces.current, b->isosurfaces.current)) return false;
  if (!same_bytes(a->ambient_occlusion.current, b->ambient_occlusion.current)) return false;
  if (!same_bytes(a->slices.current, b->slices.current)) return false;
  if (!same_bytes(a->slice_context.current, b->slice_context.current)) return false;
  if (!same_bytes(a->isosurface_context.current, b->isosurface_context.current)) return false;
  if (a->preintegration.current.mode != b->preintegration.current.mode) return false;
  if (a->gradient_opacity.current.mode != b->gradient_opacity.current.mode || !(a->gradient_opacity.current.lo == b->gradient_opacity.current.lo) ||
      !(a->gradient_opacity.current.hi == b->gradient_opacity.current.hi))
    return false;
  if (a->max_depth.current.on != b->max_depth.current.on || a->max_depth.current.width != b->max_depth.current.width || a->max_depth.current.height != b->max_depth.current.height)
    return false; // (the images are each member's copy of the same host image)
  if (a->depth_output.current.mode != b->depth_output.current.mode || !(a->depth_output.current.threshold == b->depth_output.current.threshold)) return false;
  if (a->jitter.current != b->jitter.current) return false;
  if (a->convergence.current.mode != b->convergence.current.mode || !(a->convergence.current.threshold == b->convergence.current.threshold)) return false;
  // (reconstruction: not forwarded - a group of more than one device refuses every mode but OFF)
  if (!same_bytes(a->light.current, b->light.current)) return false;
  if (!same_bytes(a->material.current, b->material.current)) return false;
  if (!same_bytes(a->clip.current, b->clip.current)) return false;
  if (a->shadow.current.mode != b->shadow.current.mode || a->shadow.current.cell != b->shadow.current.cell) return false;
  // (LDS staging: not compared - the frame is the same either way)
  // (layout choice: not compared - every layout gives the same frame; a member falls back to the general layout on its own)
  // (pipeline: not compared - both pipelines give the same frame)
  // (skipping: not compared - the frame is the same with or without)
  // the shard: every member has its own rank; the world and the tile size are the group's
  return a->shard.current.world == b->shard.current.world && a->shard.current.tw == b->shard.current.tw && a->shard.current.th == b->shard.current.th;
}
} // namespace
extern "C" {

int ovr_hip_commit(ovr_hip_renderer* r)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  if (r->group.members.size() <= 1) return commit_one(r);
  GroupLock gl(r); // every member applies the same queued values: no setter call of another thread is split between them
  // every member commits on its own thread, the leader on this one.  A failure on any member (a framebuffer that does not fit ...) leaves the members
  // on different states: the group then refuses to render until a later commit has succeeded everywhere and the members agree again
  const int e = group_run(r, GW_COMMIT, [&] { return commit_one(r); });
  bool same = true;
  for (size_t i = 1; i < r->group.members.size() && same; ++i) same = same_committed_state(r, r->group.members[i]);
  if (e || !same) {
    const std::string msg = e ? g_last_error : std::string("[hip] the members of the device group disagree on the committed state");
    r->group.broken = true;
    r->group.broken_why = msg;
    return fail(e ? e : OVR_HIP_ESTATE, msg);
  }
  r->group.broken = false;
  return 0;
}

} // extern "C"
namespace {
// consumes one queued value: true if it was set.  Recorded: that, and whether the committed value differs byte for byte from the one before
template <typename T> bool consume(commit::Changes& ch, commit::Source s, Queued<T>& q)
{
  if (!q.dirty) return false;
  const T before = q.current;
  q.update();
  ch.note(s, true, std::memcmp(&before, &q.current, sizeof(T)) != 0);
  return true;
}
bool consume(commit::Changes& ch, commit::Source s, Queued<TfnP>& q)
{
  if (!q.dirty) return false;
  const TfnP before = q.current;
  q.update();
  const TfnP& now = q.current;
  ch.note(s, true, std::memcmp(&before.lo, &now.lo, sizeof(float)) != 0 || std::memcmp(&before.hi, &now.hi, sizeof(float)) != 0 || before.colors != now.colors || before.alphas != now.alphas);
  return true;
}

// the direction table of K ambient-occlusion samples (include/ovr_hip.h): formed in float64, each component rounded to float32; on the device behind it
int upload_ao_table(ovr_hip_renderer* r, int K)
{
  const double g = 0.6180339887498949, pi = 3.141592653589793;
  r->ao_table.assign((size_t)OVR_HIP_AO_ROTATIONS * (size_t)K * 3, 0.f);
  for (int m = 0; m < OVR_HIP_AO_ROTATIONS; ++m)
    for (int j = 0; j < K; ++j) {
      const double r2 = ((double)j + 0.5) / (double)K, phi = 2.0 * pi * ((double)j * g + (double)m / 16.0);
      float* d = &r->ao_table[((size_t)m * K + j) * 3];
      d[0] = (float)(std::sqrt(r2) * std::cos(phi)); d[1] = (float)(std::sqrt(r2) * std::sin(phi)); d[2] = (float)std::sqrt(1.0 - r2);
    }
  if (K == 0) return 0; // (no frame reads the table: the buffer, if any, is kept for the next K)
  if (!r->d_ao_dirs) HIP_TRY(hipMalloc((void**)&r->d_ao_dirs, (size_t)OVR_HIP_AO_ROTATIONS * OVR_HIP_MAX_AO_SAMPLES * 3 * sizeof(float)));
  HIP_TRY(hipMemcpy(r->d_ao_dirs, r->ao_table.data(), r->ao_table.size() * sizeof(float), hipMemcpyHostToDevice)); // (a commit has finished the frame: nothing reads it)
  return 0;
}

// the first part of a commit: every queued value, in today's order, with the steps that can fail (or touch the device) where the value is consumed
int consume_queued(ovr_hip_renderer* r, commit::Changes& ch)
{
  using namespace commit;
  if (consume(ch, kFramebuffer, r->fbsize)) // device_impl.cpp:116-122
    if (int e = resize_framebuffers(r, r->fbsize.current.w, r->fbsize.current.h)) return e;
  consume(ch, kCamera, r->camera); // :125-144
  if (consume(ch, kTransferFunction, r->tfn)) { // :146-153
    if (int e = upload_tfn(r)) return e;
    update_tfn_range(r);
  }
  consume(ch, kGridConvention, r->grid_convention);
  consume(ch, kFocus, r->focus);           // :155-168
  consume(ch, kSpp, r->spp);               // :170-173
  consume(ch, kSparse, r->sparse);         // :180-183
  consume(ch, kAccumulation, r->accumulate); // :185-188
  consume(ch, kSamplingRate, r->rate);     // :190-196
  { // the projection mode, the isovalues, the AO state, the slices and their context are recorded with the shading mode: set if any of the setters was called, differs if any value differs
    const int shading = r->shading.current, projection = r->projection.current;
    const IsoP iso = r->isosurfaces.current;
    const AoP ao = r->ambient_occlusion.current;
    const SliceP sl = r->slices.current;
    const SliceContextP sc = r->slice_context.current;
    const bool set_s = r->shading.update(), set_p = r->projection.update(), set_i = r->isosurfaces.update(), set_a = r->ambient_occlusion.update(), set_l = r->slices.update();
    const IsoContextP ic = r->isosurface_context.current;
    const bool set_c = r->slice_context.update(), set_ic = r->isosurface_context.update();
    const int pm = r->preintegration.current.mode;
    const bool set_pi = r->preintegration.update();
    ch.note(kShading, set_s || set_p || set_i || set_a || set_l || set_c || set_ic,
            shading != r->shading.current || projection != r->projection.current || std::memcmp(&iso, &r->isosurfaces.current, sizeof(IsoP)) != 0 ||
              std::memcmp(&ao, &r->ambient_occlusion.current, sizeof(AoP)) != 0 || std::memcmp(&sl, &r->slices.current, sizeof(SliceP)) != 0 ||
              sc.mode != r->slice_context.current.mode || !(sc.scale == r->slice_context.current.scale) ||
              ic.mode != r->isosurface_context.current.mode || !(ic.scale == r->isosurface_context.current.scale));
    if (set_pi) ch.note(kShading, true, ch.of[kShading].differs || pm != r->preintegration.current.mode); // ovr_hip_set_preintegration: the same row - a call sets it, a changed mode differs
    {
      const GradientOpacityState go = r->gradient_opacity.current;
      if (r->gradient_opacity.update()) // ovr_hip_set_gradient_opacity: the same row - a call sets it, a changed mode or threshold differs
        ch.note(kShading, true, ch.of[kShading].differs || go.mode != r->gradient_opacity.current.mode || !(go.lo == r->gradient_opacity.current.lo) || !(go.hi == r->gradient_opacity.current.hi));
    }
    if (r->max_depth.update()) { // ovr_hip_set_max_depth: the same row - a call sets it; with an image it counts as a change, contents are not compared
      const MaxDepthState& m = r->max_depth.current;
      if (m.on) { // the image the setter queued becomes the committed one (the commit has finished the frame: nothing reads either)
        std::swap(r->d_max_depth, r->d_max_depth_queued);
        std::swap(r->max_depth_capacity, r->max_depth_queued_capacity);
      }
      ch.note(kShading, true, true);
    }
    {
      const DepthOutputState dz = r->depth_output.current;
      if (r->depth_output.update()) // ovr_hip_set_depth_output: the same row - a call sets it, a changed mode or threshold differs
        ch.note(kShading, true, ch.of[kShading].differs || dz.mode != r->depth_output.current.mode || !(dz.threshold == r->depth_output.current.threshold));
    }
    if (ao.samples != r->ambient_occlusion.current.samples) // the table follows K
      if (int e = upload_ao_table(r, r->ambient_occlusion.current.samples)) return e;
  }
  consume(ch, kJitter, r->jitter);
  {
    const int before = r->convergence.current.mode;
    ch.note(kConvergence, r->convergence.update(), r->convergence.current.mode != before);
    if (effects_of(ch, kConvergence) & kFreeConvergence) {
      HIP_TRY(hipDeviceSynchronize());
      if (int e = free_convergence(r)) return e;
    }
  }
  if (consume(ch, kReconstruction, r->reconstruction) && (effects_of(ch, kReconstruction) & kFreeReconstruction)) {
    HIP_TRY(hipDeviceSynchronize());
    if (int e = free_reconstruction(r)) return e;
  }
  {
    const LightP before = r->light.current;
    const bool set = r->light.update();
    const LightP& now = r->light.current;
    const V3 ub = unit_light(before), un = unit_light(now);
    ch.note(kLightVector, set, std::memcmp(before.dir, now.dir, sizeof(now.dir)) != 0);
    ch.note(kLightDirection, set, std::memcmp(&ub, &un, sizeof(V3)) != 0);
    ch.note(kLightIntensity, set, std::memcmp(&before.intensity, &now.intensity, sizeof(float)) != 0);
  }
  consume(ch, kMaterial, r->material);
  consume(ch, kClipBox, r->clip);
  {
    const ShadowP before = r->shadow.current;
    const bool set = r->shadow.update();
    const ShadowP& now = r->shadow.current;
    const bool mode = before.mode != now.mode;
    ch.note(kShadowMode, set, mode);
    ch.note(kShadowCell, set, before.cell != now.cell);
    ch.note(kShadowLeavesSupplied, set, mode && before.mode == OVR_HIP_SHADOWS_SUPPLIED);
    ch.note(kShadowEntersMarched, set, mode && now.mode == OVR_HIP_SHADOWS_MARCHED);
    const unsigned frees = effects_of(ch, kShadowLeavesSupplied) | effects_of(ch, kShadowEntersMarched);
    if (frees) {
      HIP_TRY(hipDeviceSynchronize());
      ShadowCacheState& c = r->shadow_cache;
      if ((frees & kFreeSuppliedLattice) && c.d_supplied) { HIP_TRY(hipFree(c.d_supplied)); c.d_supplied = nullptr; c.supplied_dims[0] = c.supplied_dims[1] = c.supplied_dims[2] = 0; }
      if ((frees & kFreeBuiltLattice) && c.d_built) { HIP_TRY(hipFree(c.d_built)); c.d_built = nullptr; c.built_cap = 0; c.built_dims[0] = c.built_dims[1] = c.built_dims[2] = 0; }
    }
  }
  consume(ch, kLdsStaging, r->lds_staging);
  consume(ch, kLayoutChoice, r->layout_choice);
  consume(ch, kPipeline, r->pipeline);
  consume(ch, kSkipping, r->skipping);
  consume(ch, kShard, r->shard);
  return 0;
}

int commit_one(ovr_hip_renderer* r)
{
  std::lock_guard<std::mutex> lk(r->mtx);
  // test hook (tests/test_round5_gpu.py): OVR_HIP_TEST_FAIL_MEMBER=k makes member k of a device group fail the commit of a framebuffer 4242 pixels wide -
  // the way a member that cannot allocate its framebuffer would - so that the group's refusal to render in mixed state can be exercised on one card
  if (r->fbsize.dirty && r->fbsize.queued.w == 4242)
    if (const char* t = getenv("OVR_HIP_TEST_FAIL_MEMBER"))
      if ((r->group.leader ? r->group.rank : 0) == atoi(t) && (r->group.leader || r->group.members.size() > 1)) {
        r->fbsize.dirty = false; // (the value is consumed, like a real failure half-way through)
        return fail(OVR_HIP_EDEVICE, "[hip] commit failed on member " + std::string(t) + " (OVR_HIP_TEST_FAIL_MEMBER)");
      }
  // what is consumed, in the reference's order (device_impl.cpp:113-197), is recorded; what follows from it is commit_plan.hpp's table.  A failed step
  // ends the consumption there: what was consumed so far takes effect, and the accumulation starts over - the state is partly applied
  commit::Changes ch;
  const int e = consume_queued(r, ch);
  commit::CommitFacts facts;
  facts.reset_pending = r->fb_reset || e != 0; // (without accumulation the flag is never consumed)
  facts.camera_dirty = r->camera_dirty;
  facts.framebuffer = r->fbsize.current.w > 0 && r->fbsize.current.h > 0;
  facts.volume = r->have_volume;
  apply_effects(r, commit::plan_commit(ch, facts));
  return e;
}
} // namespace
extern "C" {

int ovr_hip_render_async(ovr_hip_renderer* r)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  if (r->group.members.size() <= 1) return enqueue_frame(r);
  if (r->group.broken) return fail(OVR_HIP_ESTATE, "[hip] the device group is not renderable since a member failed: " + r->group.broken_why);
  // every device starts its tiles - each member's frame is enqueued by its own thread, the leader's by this one; the gather happens when the
  // frame is resolved (group_finish)
  const auto t0 = std::chrono::high_resolution_clock::now();
  const int e = group_run(r, GW_RENDER, [&] { return enqueue_frame(r); });
  r->group.host_us[0] = std::chrono::duration<double, std::micro>(std::chrono::high_resolution_clock::now() - t0).count();
  return e;
}

int ovr_hip_sync(ovr_hip_renderer* r)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  HIP_TRY(hipStreamSynchronize(r->stream())); // also covers pack / unpack / mask work enqueued after the frame
  return 0;
}

int ovr_hip_render(ovr_hip_renderer* r)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  const auto t0 = std::chrono::high_resolution_clock::now(); // optix7/device.cpp:37-42
  if (int e = ovr_hip_render_async(r)) return e;
  const auto tm = std::chrono::high_resolution_clock::now();
  if (int e = finish_frame(r)) return e;
  const auto t1 = std::chrono::high_resolution_clock::now();
  const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
  static const bool slow_trace = getenv("OVR_HIP_SLOW_FRAMES") != nullptr; // diagnostic: where a frame that took > 20 ms of host time spent it
  if (slow_trace && ms > 20.0)
    fprintf(stderr, "[hip] slow frame %d: enqueue %.2f ms, wait + finish %.2f ms (kernels %.2f ms)\n", r->frame_index, std::chrono::duration<double, std::milli>(tm - t0).count(),
            std::chrono::duration<double, std::milli>(t1 - tm).count(), r->stats.kernel_ms);
  // diagnostic: OVR_HIP_FRAME_TIMING=n prints, every n frames, the mean host time of a blocking render() split into enqueue / wait, next to the
  // frame's device time between its first and last event - the difference is launch latency, the counter read-back and the wake-up
  static const int timing_every = getenv("OVR_HIP_FRAME_TIMING") ? atoi(getenv("OVR_HIP_FRAME_TIMING")) : 0;
  if (timing_every > 0) {
    static thread_local double acc[3] = { 0, 0, 0 };
    static thread_local int n_acc = 0;
    acc[0] += std::chrono::duration<double, std::milli>(tm - t0).count(); acc[1] += std::chrono::duration<double, std::milli>(t1 - tm).count(); acc[2] += r->stats.kernel_ms;
    if (++n_acc == timing_every) {
      fprintf(stderr, "[hip] %d frames: render() %.4f ms = enqueue %.4f + wait %.4f ; device first-to-last event %.4f ms ; outside the events %.4f ms\n", n_acc,
              (acc[0] + acc[1]) / n_acc, acc[0] / n_acc, acc[1] / n_acc, acc[2] / n_acc, (acc[0] + acc[1] - acc[2]) / n_acc);
      acc[0] = acc[1] = acc[2] = 0; n_acc = 0;
    }
  }
  r->stats.render_ms = ms;
  r->render_time_ms += ms;
  return 0;
}

int ovr_hip_mapframe(ovr_hip_renderer* r, int mem_kind, const float** rgba, size_t* rgba_bytes, const float** grad, size_t* grad_bytes)
{
  if (!r || !rgba || !rgba_bytes) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_mapframe: null argument");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  const size_t n = r->fb_pixels;
  const int c = r->cur;
  if (mem_kind == OVR_HIP_MEM_DEVICE) {
    *rgba = r->d_rgba[c];
    *rgba_bytes = n * 4 * sizeof(float);
    if (grad) *grad = r->d_grad[c];
    if (grad_bytes) *grad_bytes = n * 3 * sizeof(float);
    return 0;
  }
  if (mem_kind != OVR_HIP_MEM_HOST) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_mapframe: bad mem_kind");
  if (n == 0) { *rgba = nullptr; *rgba_bytes = 0; if (grad) *grad = nullptr; if (grad_bytes) *grad_bytes = 0; return 0; }
  hipStream_t st = r->stream();
  // the mirrors start as zeros and only the rectangle the box projects into is ever copied (refresh_mirror): C3's oblique view moves 22 of
  // the frame's 58 MB, 0.4 instead of 1.04 ms per mapped frame (profiles/r03_notes.md)
  if (!r->h_rgba[c]) {
    HIP_TRY(hipHostMalloc((void**)&r->h_rgba[c], n * 4 * sizeof(float), hipHostMallocDefault));
    std::memset(r->h_rgba[c], 0, n * 4 * sizeof(float));
    for (int k = 0; k < 4; ++k) r->h_rgba_rect[c][k] = 0;
  }
  if (int e = refresh_mirror(r, r->h_rgba[c], r->d_rgba[c], 4, r->d_rect[c], r->h_rgba_rect[c], st)) return e;
  if (grad) {
    if (!r->h_grad[c]) {
      HIP_TRY(hipHostMalloc((void**)&r->h_grad[c], n * 3 * sizeof(float), hipHostMallocDefault));
      std::memset(r->h_grad[c], 0, n * 3 * sizeof(float));
      for (int k = 0; k < 4; ++k) r->h_grad_rect[c][k] = 0;
    }
    if (int e = refresh_mirror(r, r->h_grad[c], r->d_grad[c], 3, r->d_rect[c], r->h_grad_rect[c], st)) return e;
  }
  HIP_TRY(hipStreamSynchronize(st));
  *rgba = r->h_rgba[c];
  *rgba_bytes = n * 4 * sizeof(float);
  if (grad) *grad = r->h_grad[c];
  if (grad_bytes) *grad_bytes = n * 3 * sizeof(float);
  return 0;
}

int ovr_hip_mapframe_rgba8(ovr_hip_renderer* r, int mem_kind, int flip_vertical, const uint32_t** rgba8, size_t* bytes)
{
  if (!r || !rgba8 || !bytes) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_mapframe_rgba8: null argument");
  if (mem_kind != OVR_HIP_MEM_DEVICE && mem_kind != OVR_HIP_MEM_HOST) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_mapframe_rgba8: bad mem_kind");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  const size_t n = r->fb_pixels;
  *rgba8 = nullptr;
  *bytes = 0;
  if (n == 0) return 0;
  hipStream_t st = r->stream();
  if (!r->d_rgba8) HIP_TRY(hipMalloc((void**)&r->d_rgba8, n * sizeof(uint32_t)));
  HIP_TRY(launch_rgba8(r->d_rgba[r->cur], r->d_rgba8, r->fbsize.current.w, r->fbsize.current.h, flip_vertical ? 1 : 0, st));
  if (mem_kind == OVR_HIP_MEM_HOST) {
    if (!r->h_rgba8) HIP_TRY(hipHostMalloc((void**)&r->h_rgba8, n * sizeof(uint32_t), hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(r->h_rgba8, r->d_rgba8, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  *rgba8 = mem_kind == OVR_HIP_MEM_HOST ? r->h_rgba8 : r->d_rgba8;
  *bytes = n * sizeof(uint32_t);
  return 0;
}

int ovr_hip_mapframe_rgba16f(ovr_hip_renderer* r, int mem_kind, int flip_vertical, const uint16_t** rgba16f, size_t* bytes)
{
  if (!r || !rgba16f || !bytes) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_mapframe_rgba16f: null argument");
  if (mem_kind != OVR_HIP_MEM_DEVICE && mem_kind != OVR_HIP_MEM_HOST) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_mapframe_rgba16f: bad mem_kind");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  const size_t n = r->fb_pixels;
  *rgba16f = nullptr;
  *bytes = 0;
  if (n == 0) return 0;
  hipStream_t st = r->stream();
  if (!r->d_rgba16f) HIP_TRY(hipMalloc((void**)&r->d_rgba16f, n * 4 * sizeof(uint16_t)));
  HIP_TRY(launch_rgba16f(r->d_rgba[r->cur], r->d_rgba16f, r->fbsize.current.w, r->fbsize.current.h, flip_vertical ? 1 : 0, st));
  if (mem_kind == OVR_HIP_MEM_HOST) {
    if (!r->h_rgba16f) HIP_TRY(hipHostMalloc((void**)&r->h_rgba16f, n * 4 * sizeof(uint16_t), hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(r->h_rgba16f, r->d_rgba16f, n * 4 * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  *rgba16f = mem_kind == OVR_HIP_MEM_HOST ? r->h_rgba16f : r->d_rgba16f;
  *bytes = n * 4 * sizeof(uint16_t);
  return 0;
}

int ovr_hip_get_volume_info(const ovr_hip_renderer* r, ovr_hip_volume_info* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_volume_info: null argument");
  if (!r->have_volume) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_volume_info: no volume was set");
  out->dims[0] = r->vd.nx; out->dims[1] = r->vd.ny; out->dims[2] = r->vd.nz;
  out->value_type = r->value_type;
  out->resident_bytes = (uint64_t)r->volume_bytes;
  out->data_lower = r->data_lower;
  out->data_upper = r->data_upper;
  out->tf_lower = r->P.tf_lower;
  out->tf_upper = r->P.tf_upper;
  return 0;
}

int ovr_hip_swap(ovr_hip_renderer* r)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  HIP_TRY(hipStreamSynchronize(r->stream())); // device_impl.cpp:105
  r->cur = (r->cur + 1) % 2;                  // safe_swap, optix7_common.h:366-370
  if (r->group.members.size() > 1) return group_run(r, GW_SWAP);
  return 0;
}

double ovr_hip_render_time_ms(const ovr_hip_renderer* r) { return r ? r->render_time_ms : 0.0; }

int ovr_hip_get_stats(const ovr_hip_renderer* r, ovr_hip_stats* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_stats: null argument");
  if (r->async_pending) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_stats: a frame is still in flight (call ovr_hip_sync)");
  *out = r->stats;
  return 0;
}

namespace {
void convergence_of(const ovr_hip_renderer* m, ovr_hip_convergence* out)
{
  const ConvP& c = m->convergence.current;
  out->threshold = c.threshold;
  out->mode = c.mode;
  out->valid = m->conv.valid ? 1 : 0;
  out->error = m->conv.valid ? m->conv.error : INFINITY;
  out->frames = m->conv.valid ? m->conv.frames : 0;
  const bool adaptive = c.mode == OVR_HIP_CONVERGENCE_ADAPTIVE;
  out->blocks = c.mode != OVR_HIP_CONVERGENCE_OFF ? (int32_t)m->sched.n_work : 0;
  out->retired_blocks = adaptive ? (int32_t)m->conv.retired : 0;
  out->active_blocks = out->blocks - out->retired_blocks;
}
// the renderer a diagnostic download addresses: member k of a device group, the renderer itself otherwise
ovr_hip_renderer* member_of(ovr_hip_renderer* r, int32_t member)
{
  const int n = r->group.members.size() > 1 ? (int)r->group.members.size() : 1;
  if (member < 0 || member >= n) return nullptr;
  return n > 1 ? r->group.members[(size_t)member] : r;
}
} // namespace

int ovr_hip_get_convergence(const ovr_hip_renderer* r, ovr_hip_convergence* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_convergence: null argument");
  if (r->async_pending) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_convergence: a frame is still in flight (call ovr_hip_sync)");
  convergence_of(r, out);
  for (size_t i = 1; i < r->group.members.size(); ++i) { // a device group: the largest error, the blocks of all members
    ovr_hip_convergence a;
    convergence_of(r->group.members[i], &a);
    out->valid = out->valid && a.valid;
    out->error = std::max(out->error, a.error);
    out->blocks += a.blocks; out->active_blocks += a.active_blocks; out->retired_blocks += a.retired_blocks;
  }
  if (!out->valid) { out->error = INFINITY; out->frames = 0; }
  return 0;
}

int ovr_hip_get_convergence_blocks(ovr_hip_renderer* r, int32_t member, int32_t dims[2], float* error_host, int32_t* frames_host, size_t capacity_blocks)
{
  if (!r || !dims) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_convergence_blocks: null argument");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  ovr_hip_renderer* m = member_of(r, member);
  if (!m) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_convergence_blocks: no such member");
  dims[0] = (m->fbsize.current.w + 7) / 8; dims[1] = (m->fbsize.current.h + 7) / 8;
  const size_t blocks = (size_t)dims[0] * (size_t)dims[1];
  if (!error_host && !frames_host) return 0;
  if (capacity_blocks < blocks) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_convergence_blocks: output too small");
  if (!m->conv.d_error || m->conv.blocks != blocks) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_convergence_blocks: no frame was rendered with the convergence estimate on");
  if (blocks == 0) return 0;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream()));
  if (error_host) HIP_TRY(hipMemcpy(error_host, m->conv.d_error, blocks * sizeof(float), hipMemcpyDeviceToHost));
  if (frames_host) HIP_TRY(hipMemcpy(frames_host, m->conv.d_frames, blocks * sizeof(int32_t), hipMemcpyDeviceToHost));
  return set_device(r);
}

int ovr_hip_get_accumulation(ovr_hip_renderer* r, int32_t member, int32_t which, float* host, size_t capacity_floats)
{
  if (!r || !host || (which != 0 && which != 1)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_accumulation: bad argument");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  ovr_hip_renderer* m = member_of(r, member);
  if (!m) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_accumulation: no such member");
  const size_t floats = m->fb_pixels * 4;
  if (capacity_floats < floats) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_accumulation: output too small");
  const float* src = which == 0 ? m->d_accum : m->conv.d_accum_half;
  if (!src) return fail(OVR_HIP_ESTATE, which == 0 ? "[hip] ovr_hip_get_accumulation: no framebuffer" : "[hip] ovr_hip_get_accumulation: no frame was rendered with the convergence estimate on");
  if (floats == 0) return 0;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream()));
  HIP_TRY(hipMemcpy(host, src, floats * sizeof(float), hipMemcpyDeviceToHost));
  return set_device(r);
}

int ovr_hip_get_reconstruction(const ovr_hip_renderer* r, ovr_hip_reconstruction* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_reconstruction: null argument");
  if (r->async_pending) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_reconstruction: a frame is still in flight (call ovr_hip_sync)");
  *out = r->recon.info;
  out->mode = r->reconstruction.current;
  return 0;
}

namespace {
int recon_read(ovr_hip_renderer* r, const char* what, bool gradient, float* host, size_t capacity_floats)
{
  if (!r || !host) return fail(OVR_HIP_EINVAL, std::string("[hip] ") + what + ": null argument");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  const size_t floats = r->fb_pixels * (gradient ? 3 : 1);
  if (capacity_floats < floats) return fail(OVR_HIP_EINVAL, std::string("[hip] ") + what + ": output too small");
  const float* src = gradient ? r->recon.d_grad : r->recon.d_count;
  if (!src) return fail(OVR_HIP_ESTATE, std::string("[hip] ") + what + ": no frame was rendered with the reconstruction on");
  if (gradient && !r->recon.accumulated) return fail(OVR_HIP_ESTATE, std::string("[hip] ") + what + ": the last reconstructed frame did not accumulate");
  if (floats == 0) return 0;
  HIP_TRY(hipStreamSynchronize(r->stream()));
  HIP_TRY(hipMemcpy(host, src, floats * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}
} // namespace

int ovr_hip_get_reconstruction_weights(ovr_hip_renderer* r, float* host, size_t capacity_floats)
{
  return recon_read(r, "ovr_hip_get_reconstruction_weights", false, host, capacity_floats);
}

int ovr_hip_get_reconstruction_gradient(ovr_hip_renderer* r, float* host, size_t capacity_floats)
{
  return recon_read(r, "ovr_hip_get_reconstruction_gradient", true, host, capacity_floats);
}

int ovr_hip_reconstruct_image(ovr_hip_renderer* r, float* rgba_device, float* grad_device, const float* weight_device, int32_t width, int32_t height)
{
  if (!r || !rgba_device || !weight_device) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_reconstruct_image: null argument");
  if (width < 0 || height < 0 || (int64_t)width * (int64_t)height > (int64_t)0x7fffffff) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_reconstruct_image: bad image size");
  if (width == 0 || height == 0) return 0;
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  ReconParams c{};
  c.width = width; c.height = height;
  const size_t texels = recon_plan(c);
  float4* pyramid = nullptr;
  unsigned int* words = nullptr;
  HIP_TRY(hipMalloc((void**)&pyramid, std::max<size_t>(texels, 1) * 2 * sizeof(float4)));
  if (hipMalloc((void**)&words, kReconWords * sizeof(unsigned int)) != hipSuccess) { (void)hipFree(pyramid); return fail(OVR_HIP_EDEVICE, "[hip] ovr_hip_reconstruct_image: out of device memory"); }
  hipStream_t st = r->stream();
  c.rgba = rgba_device; c.grad = grad_device; c.count = weight_device;
  c.pyramid = pyramid; c.words = words; c.sub_capacity = 0xffffffffu;
  hipError_t e = hipMemsetAsync(words, 0, kReconWords * sizeof(unsigned int), st);
  if (e == hipSuccess) e = launch_reconstruct(c, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(pyramid);
  (void)hipFree(words);
  if (e != hipSuccess) return fail(OVR_HIP_EDEVICE, std::string("[hip] ovr_hip_reconstruct_image: ") + hipGetErrorString(e));
  return 0;
}

int ovr_hip_get_macrocells(ovr_hip_renderer* r, int32_t dims[3], float* minmax_host, float* majorant_host, size_t capacity_cells)
{
  if (!r || !dims) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_macrocells: null argument");
  if (!r->have_volume || !r->have_tfn) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_macrocells: needs a volume and a transfer function");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  dims[0] = (r->vd.nx + 15) / 16; dims[1] = (r->vd.ny + 15) / 16; dims[2] = (r->vd.nz + 15) / 16;
  const size_t cells = (size_t)dims[0] * dims[1] * dims[2];
  if (!minmax_host && !majorant_host) return 0;
  if (capacity_cells < cells) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_macrocells: output too small");
  hipStream_t st = r->stream();
  if (int e = update_macrocells(r, st)) return e;
  HIP_TRY(hipStreamSynchronize(st));
  if (minmax_host) HIP_TRY(hipMemcpy(minmax_host, r->d_mc_minmax, cells * 2 * sizeof(float), hipMemcpyDeviceToHost));
  if (majorant_host) HIP_TRY(hipMemcpy(majorant_host, r->d_mc_majorant, cells * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int ovr_hip_owned_tiles(const ovr_hip_renderer* r, int32_t rank, int32_t* n_tiles)
{
  if (!r || !n_tiles) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_owned_tiles: null argument");
  const ShardP& s = r->shard.current;
  if (rank < 0 || rank >= s.world) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_owned_tiles: rank out of range");
  *n_tiles = count_owned_tiles(r->fbsize.current.w, r->fbsize.current.h, s.tw, s.th, rank, s.world);
  return 0;
}

int ovr_hip_pack_tiles(ovr_hip_renderer* r, float* dst, size_t dst_bytes)
{
  if (!r || !dst) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_pack_tiles: null argument");
  if (r->group.members.size() > 1) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_pack_tiles: a device group gathers its tiles itself");
  if (int e = set_device(r)) return e;
  // A frame of the pooled pipeline may still have to be rendered again (request-pool overflow: nothing was written to the
  // framebuffer and only the host can grow the pool).  Until the pool has proven roomy for this configuration (the last frame
  // used at most half of it) the frame is resolved before its tiles are packed; after that the pack is enqueued right behind
  // the frame, and should the improbable happen - an overflow after all - ovr_hip_stats.stale_tiles tells the caller.
  if (r->async_pending && r->P.pool.reqs) {
    if (!r->pool_roomy) { if (int e = finish_frame(r)) return e; }
    else r->packed_early = true; // steady state: the pack runs right behind the frame, nothing waits on the host
  }
  const ShardP& s = r->shard.current;
  const int W = r->fbsize.current.w, H = r->fbsize.current.h;
  const size_t need = (size_t)count_owned_tiles(W, H, s.tw, s.th, s.rank, s.world) * s.tw * s.th * 4 * sizeof(float);
  if (dst_bytes < need) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_pack_tiles: destination too small");
  HIP_TRY(launch_pack_tiles(r->d_rgba[r->cur], dst, W, H, s.tw, s.th, s.rank, s.world, r->stream()));
  return 0;
}

int ovr_hip_unpack_tiles(ovr_hip_renderer* r, int32_t src_rank, const float* src, size_t src_bytes, float* frame, size_t frame_bytes)
{
  if (!r || !src || !frame) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_unpack_tiles: null argument");
  if (int e = set_device(r)) return e;
  const ShardP& s = r->shard.current;
  const int W = r->fbsize.current.w, H = r->fbsize.current.h;
  if (src_rank < 0 || src_rank >= s.world) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_unpack_tiles: rank out of range");
  const size_t need = (size_t)count_owned_tiles(W, H, s.tw, s.th, src_rank, s.world) * s.tw * s.th * 4 * sizeof(float);
  if (src_bytes < need) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_unpack_tiles: source too small");
  if (frame_bytes < (size_t)W * H * 4 * sizeof(float)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_unpack_tiles: frame too small");
  HIP_TRY(launch_unpack_tiles(src, frame, W, H, s.tw, s.th, src_rank, s.world, 0, r->stream()));
  return 0;
}

int ovr_hip_unpack_all_tiles(ovr_hip_renderer* r, const float* src, size_t rank_stride_bytes, size_t src_bytes, float* frame, size_t frame_bytes)
{
  if (!r || !src || !frame) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_unpack_all_tiles: null argument");
  if (int e = set_device(r)) return e;
  const ShardP& s = r->shard.current;
  const int W = r->fbsize.current.w, H = r->fbsize.current.h;
  size_t need = 0;
  for (int k = 0; k < s.world; ++k)
    need = std::max(need, (size_t)count_owned_tiles(W, H, s.tw, s.th, k, s.world) * s.tw * s.th * 4 * sizeof(float));
  if (rank_stride_bytes % 16 != 0 || rank_stride_bytes < need) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_unpack_all_tiles: rank stride too small or not a multiple of 16");
  if (src_bytes < rank_stride_bytes * (size_t)(s.world - 1) + need) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_unpack_all_tiles: source too small");
  if (frame_bytes < (size_t)W * H * 4 * sizeof(float)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_unpack_all_tiles: frame too small");
  HIP_TRY(launch_unpack_tiles(src, frame, W, H, s.tw, s.th, -1, s.world, rank_stride_bytes / sizeof(float), r->stream()));
  return 0;
}

int ovr_hip_sparse_mask(ovr_hip_renderer* r, int32_t frame_index, int32_t* out_xy, size_t out_bytes, int64_t* n_out)
{
  if (!r || !out_xy || !n_out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_sparse_mask: null argument");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  if (!r->d_noise) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_sparse_mask: no noise tile was set");
  const int W = r->fbsize.current.w, H = r->fbsize.current.h;
  if (W <= 0 || H <= 0) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_sparse_mask: framebuffer size not committed");
  if (out_bytes < (size_t)W * H * 2 * sizeof(int32_t)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_sparse_mask: output too small");
  if (int e = ensure_sparse_buffers(r)) return e;
  hipStream_t st = r->stream();
  HIP_TRY(launch_sparse_mask(make_mask_params(r, frame_index, out_xy), st));
  unsigned long long cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, r->d_sparse_count, sizeof(cnt), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *n_out = (int64_t)cnt;
  return 0;
}

int ovr_hip_pow_floats(ovr_hip_renderer* r, const float* x, const float* y, float* out, int64_t n, int32_t which)
{
  if (!r || !x || !y || !out || n < 0 || which < 0 || which > 1) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_pow_floats: bad arguments");
  if (int e = set_device(r)) return e;
  HIP_TRY(launch_pow(x, y, out, n, which, r->stream()));
  HIP_TRY(hipStreamSynchronize(r->stream()));
  return 0;
}

int ovr_hip_built_for_exact_parity(void) { return built_for_exact_parity(); }

int ovr_hip_shade_floats(ovr_hip_renderer* r, const float* normal_w, const float* pos, const float* shadow, float* out, int64_t n)
{
  if (!r || !normal_w || !pos || !shadow || !out || n < 0) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_shade_floats: bad arguments");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  HIP_TRY(launch_shade_floats(r->P, normal_w, pos, shadow, out, n, r->stream())); // the committed light, material and camera position
  HIP_TRY(hipStreamSynchronize(r->stream()));
  return 0;
}

int ovr_hip_clip_intervals(ovr_hip_renderer* r, const float* org, const float* dir, float* t0t1hit, int64_t n)
{
  if (!r || !org || !dir || !t0t1hit || n < 0) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_clip_intervals: bad arguments");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  if (!r->have_volume) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_clip_intervals: no volume was set");
  HIP_TRY(launch_clip_intervals(r->P, org, dir, t0t1hit, n, r->stream())); // the committed volume transform and clip box
  HIP_TRY(hipStreamSynchronize(r->stream()));
  return 0;
}

int ovr_hip_shadow_floats(ovr_hip_renderer* r, const float* pos, float* out, int64_t n, int32_t which)
{
  if (!r || !pos || !out || n < 0 || (which != 0 && which != 1)) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_shadow_floats: bad arguments");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  if (!r->have_volume || !r->have_tfn) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_shadow_floats: needs a volume and a transfer function");
  hipStream_t st = r->stream();
  RayMarchParams q = r->P;
  fill_shadow_params(r, q); // the committed sampling rate, transfer function and the general layout, as a frame sets them
  if (which == 0) {
    if (r->tf_copy_pending) { HIP_TRY(hipStreamWaitEvent(st, r->ev_tf, 0)); r->tf_copy_pending = false; }
    ShadowBuildArgs a{};
    a.out = out;
    a.pos = pos;
    a.n = n;
    HIP_TRY(launch_shadow_cache(q, a, st));
  }
  else {
    if (r->shadow.current.mode == OVR_HIP_SHADOWS_MARCHED) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_shadow_floats: the committed mode is MARCHED - there is no lattice to look up");
    if (int e = ensure_shadow_cache(r, q, st)) return e;
    HIP_TRY(launch_shadow_lookup(q, pos, out, n, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

// the known-answer ray queries (the table's seven and the pre-integrated march's): one path, walked by the entry's row of host/ray_query.hpp - what must be committed, which parameters it binds, its record
namespace {
static_assert(kQueryEinval == OVR_HIP_EINVAL && kQueryEstate == OVR_HIP_ESTATE && kQueryRotations == OVR_HIP_AO_ROTATIONS && kProjectMaximum == OVR_HIP_PROJECT_MAXIMUM
                && kProjectMean == OVR_HIP_PROJECT_MEAN,
              "host/ray_query.hpp restates include/ovr_hip.h");
int ray_query(ovr_hip_renderer* r, int id, const float* org, const float* dir, float* out, int64_t n, int32_t mode = 0, int32_t max_events = 0, int32_t rotation = 0,
              int32_t range_skipping = 0, const float* depth = nullptr, float threshold = 0.f) // (0: what the entry does not take)
{
  const RayQuery& d = ray_query_row(id);
  RayQueryCall c;
  c.org = org; c.dir = dir; c.out = out; c.n = n;
  c.mode = mode; c.max_events = max_events; c.rotation = rotation; c.range_skipping = range_skipping;
  c.depth = depth;
  c.threshold = threshold;
  if (const QueryStatus s = ray_query_arguments(d, r != nullptr, c); s.code) return fail(s.code, s.message);
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  QueryFacts f;
  f.volume = r->have_volume;
  f.slices = r->slices.current.n;
  f.isovalues = r->isosurfaces.current.n;
  f.slice_context = r->slice_context.current.mode == OVR_HIP_SLICE_CONTEXT_FRONT;
  f.isosurface_context = r->isosurface_context.current.mode == OVR_HIP_ISO_CONTEXT_VOLUME;
  f.ao_samples = r->ambient_occlusion.current.samples;
  f.transfer_function = r->d_tf_color && r->d_tf_alpha;
  f.ranges = projection_ranges(r) != nullptr;
  f.preintegration = r->preintegration.current.mode == OVR_HIP_PREINTEGRATION_SEGMENTS;
  f.gradient_opacity = r->gradient_opacity.current.mode == OVR_HIP_GRADIENT_OPACITY_RAMP;
  if (const QueryStatus s = ray_query_preconditions(d, f, c.range_skipping != 0); s.code) return fail(s.code, s.message);
  RayMarchParams q = r->P;
  fill_shadow_params(r, q); // the committed sampling rate and the general layout, as a frame sets them (the tables are read by the context kernels alone)
  if (d.needs_tf) { // the committed tables, as a frame binds them
    q.tf_color = r->d_tf_color; q.tf_alpha = r->d_tf_alpha;
    q.n_color = r->n_color; q.n_alpha = r->n_alpha;
  }
  if (d.needs == QueryNeeds::Slices) fill_slice_params(r, q);
  if (d.needs == QueryNeeds::Isovalues) fill_isosurface_params(r, q);
  if (d.takes_range_skipping) q.mc_ranges = projection_ranges(r);
  if (d.needs_preintegration) { // the unshaded march's node table, whatever frame kind and shading mode are committed
    q.shading = 0; q.projection = 0; q.iso_n = 0; q.slice_n = 0; q.ao_samples = 0;
    q.pool = PoolDesc{}; q.majorant = nullptr; q.sparse_xy = nullptr; q.schedule = nullptr; q.n_schedule = 0;
    if (int e = bind_preintegration(r, q)) return e;
  }
  if (d.needs_gradient_opacity) { // the march's plan under the asked shading, whatever frame kind and shading mode are committed
    q.projection = 0; q.iso_n = 0; q.slice_n = 0; q.ao_samples = 0;
    q.pool = PoolDesc{}; q.majorant = nullptr; q.sparse_xy = nullptr; q.schedule = nullptr; q.n_schedule = 0;
    fill_gradient_opacity_params(r, q, true);
  }
  if (d.takes_depth) { // the march's plan under the asked shading, whatever frame kind and shading mode are committed
    q.projection = 0; q.iso_n = 0; q.slice_n = 0; q.ao_samples = 0;
    q.pool = PoolDesc{}; q.majorant = nullptr; q.sparse_xy = nullptr; q.schedule = nullptr; q.n_schedule = 0;
  }
  HIP_TRY(launch_ray_query(id, q, c, r->stream()));
  HIP_TRY(hipStreamSynchronize(r->stream()));
  return 0;
}
} // namespace

int ovr_hip_project_floats(ovr_hip_renderer* r, const float* org, const float* dir, float* out, int64_t n, int32_t mode, int32_t range_skipping)
{
  return ray_query(r, kQueryProject, org, dir, out, n, mode, 0, 0, range_skipping);
}

int ovr_hip_slice_floats(ovr_hip_renderer* r, const float* org, const float* dir, float* out, int64_t n, int32_t range_skipping)
{
  return ray_query(r, kQuerySlice, org, dir, out, n, 0, 0, 0, range_skipping);
}

int ovr_hip_slice_context_floats(ovr_hip_renderer* r, const float* org, const float* dir, float* out, int64_t n)
{
  return ray_query(r, kQuerySliceContext, org, dir, out, n);
}

int ovr_hip_preintegrated_floats(ovr_hip_renderer* r, const float* org, const float* dir, float* out, int64_t n)
{
  return ray_query(r, kQueryPreintegrated, org, dir, out, n);
}

int ovr_hip_gradient_opacity_floats(ovr_hip_renderer* r, const float* org, const float* dir, float* out, int64_t n, int32_t shade)
{
  return ray_query(r, kQueryGradientOpacity, org, dir, out, n, shade);
}

int ovr_hip_max_depth_floats(ovr_hip_renderer* r, const float* org, const float* dir, const float* depth, float* out, int64_t n, int32_t shade)
{
  return ray_query(r, kQueryMaxDepth, org, dir, out, n, shade, 0, 0, 0, depth);
}

int ovr_hip_depth_output_floats(ovr_hip_renderer* r, const float* org, const float* dir, const float* depth_or_null, float* out, int64_t n, int32_t shade, float threshold)
{
  return ray_query(r, kQueryDepthOutput, org, dir, out, n, shade, 0, 0, 0, depth_or_null, threshold);
}

int ovr_hip_isosurface_floats(ovr_hip_renderer* r, const float* org, const float* dir, float* out, int64_t n, int32_t range_skipping)
{
  return ray_query(r, kQueryIsosurface, org, dir, out, n, 0, 0, 0, range_skipping);
}

int ovr_hip_isosurface_layers_floats(ovr_hip_renderer* r, const float* org, const float* dir, float* out, int64_t n, int32_t max_events, int32_t range_skipping)
{
  return ray_query(r, kQueryIsosurfaceLayers, org, dir, out, n, 0, max_events, 0, range_skipping);
}

int ovr_hip_isosurface_context_floats(ovr_hip_renderer* r, const float* org, const float* dir, float* out, int64_t n, int32_t max_events)
{
  return ray_query(r, kQueryIsosurfaceContext, org, dir, out, n, 0, max_events);
}

int ovr_hip_isosurface_ao_floats(ovr_hip_renderer* r, const float* org, const float* dir, float* out, int64_t n, int32_t max_events, int32_t rotation, int32_t range_skipping)
{
  return ray_query(r, kQueryIsosurfaceAo, org, dir, out, n, 0, max_events, rotation, range_skipping);
}

int ovr_hip_camera_rays(ovr_hip_renderer* r, int32_t frame_index, int32_t sample, float* org_dir, size_t capacity_floats)
{
  if (!r || !org_dir || frame_index < 1) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_camera_rays: bad arguments");
  if (int e = set_device(r)) return e;
  if (int e = finish_frame(r)) return e;
  const int W = r->fbsize.current.w, H = r->fbsize.current.h;
  if (W <= 0 || H <= 0 || r->camera_dirty) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_camera_rays: no framebuffer size is committed");
  if (sample < 0 || sample >= r->spp.current) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_camera_rays: the sample lies outside 0 ... spp - 1");
  if (capacity_floats < (size_t)W * (size_t)H * 6) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_camera_rays: the buffer holds fewer than width x height x 6 floats");
  if (r->jitter.current == 1 && !r->d_noise) return fail(OVR_HIP_ESTATE, "[hip] blue-noise pixel jitter enabled but no noise tile was set (ovr_hip_set_noise_tile)");
  RayMarchParams q = r->P; // the committed camera; the frame's size, sampling and jitter as fill_target_params / fill_table_params set them
  q.width = W; q.height = H;
  q.frame_index = frame_index;
  q.spp = r->spp.current;
  q.jitter_mode = r->jitter.current;
  q.jitter_noise = r->d_noise;
  q.jitter_xy = r->noise_xy;
  HIP_TRY(launch_camera_rays(q, sample, org_dir, r->stream()));
  HIP_TRY(hipStreamSynchronize(r->stream()));
  return 0;
}

int ovr_hip_tea_floats(ovr_hip_renderer* r, uint32_t* v0v1, float* out, int64_t n)
{
  if (!r || !v0v1 || !out || n < 0) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_tea_floats: bad arguments");
  if (int e = set_device(r)) return e;
  HIP_TRY(launch_tea(v0v1, out, n, r->stream()));
  HIP_TRY(hipStreamSynchronize(r->stream()));
  return 0;
}

} // extern "C"
