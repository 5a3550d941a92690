// frame.cpp - one renderer's frame: enqueue_frame fills RayMarchParams step by step and launches, finish_frame_one reads the counters back and
// feeds the automatic policies (policy.hpp).  Mirrors Impl::render of the reference's GPU device (device_impl.cpp:199-269).
#include "state.hpp"

#include <cstdio>
#include <cstdlib>

namespace ovrhip {
namespace host {

static_assert(policy::kGeneral == LAYOUT_GENERAL && policy::kThin == LAYOUT_THIN && policy::kThinT == LAYOUT_THIN_T && policy::kQuad == LAYOUT_QUAD
              && policy::kLayoutCount == kLayouts && policy::kPoolSubCount == kPoolSubs, "policy.hpp restates ovr_hip_kernels.h");


// Shade order by light beams (PoolDesc): beams of about OVR_HIP_SHADE_BEAM voxels (default 32) across - the bricks one beam's shadow rays sweep have
// to stay in one XCD's 4 MB L2 while its runs are shaded (measured on C3: 16 / 32 / 64 voxels -> shade 0.958 / 0.937 / 0.998 ms; creation order 1.094);
// OVR_HIP_SHADE_ORDER=0: creation order (rounds 1-4).  Called once RayMarchParams holds the frame's light and volume transform.
static void shade_order_params(ovr_hip_renderer* r, PoolDesc& pd)
{
  const float beam = r->shade_beam;
  pd.order_grid = 0;
  if (!r->shade_order_on || !pd.order || !pd.order_key || !pd.order_ws) { pd.order = nullptr; return; }
  const RayMarchParams& P = r->P;
  const double diag = std::sqrt((double)r->vd.nx * r->vd.nx + (double)r->vd.ny * r->vd.ny + (double)r->vd.nz * r->vd.nz);
  const int G = diag <= 32.0 * beam ? 32 : diag <= 64.0 * beam ? 64 : 128;
  // two unit vectors perpendicular to the light: U = L x e_k (k = L's smallest component), V = L x U
  const double L[3] = { P.light.x, P.light.y, P.light.z };
  const int k = std::fabs(L[0]) <= std::fabs(L[1]) && std::fabs(L[0]) <= std::fabs(L[2]) ? 0 : std::fabs(L[1]) <= std::fabs(L[2]) ? 1 : 2;
  double U[3] = { 0, 0, 0 }, V[3];
  U[(k + 1) % 3] = L[(k + 2) % 3]; U[(k + 2) % 3] = -L[(k + 1) % 3];
  const double un = std::sqrt(U[0] * U[0] + U[1] * U[1] + U[2] * U[2]);
  if (!(un > 0.0)) { pd.order = nullptr; return; }
  for (double& u : U) u /= un;
  V[0] = L[1] * U[2] - L[2] * U[1]; V[1] = L[2] * U[0] - L[0] * U[2]; V[2] = L[0] * U[1] - L[1] * U[0];
  // the volume's box in world space (object = world * inv_scale + wto_p): centre and half diagonal
  const double sx = 1.0 / P.inv_scale.x, sy = 1.0 / P.inv_scale.y, sz = 1.0 / P.inv_scale.z;
  const double c[3] = { (0.5 - P.wto_p.x) * sx, (0.5 - P.wto_p.y) * sy, (0.5 - P.wto_p.z) * sz };
  const double R = 0.5 * std::sqrt(sx * sx + sy * sy + sz * sz), s = (double)G / (2.0 * R);
  if (!std::isfinite(s) || !(s > 0.0)) { pd.order = nullptr; return; }
  for (int i = 0; i < 3; ++i) { pd.order_u[i] = (float)(U[i] * s); pd.order_v[i] = (float)(V[i] * s); }
  pd.order_u[3] = (float)((R - (c[0] * U[0] + c[1] * U[1] + c[2] * U[2])) * s);
  pd.order_v[3] = (float)((R - (c[0] * V[0] + c[1] * V[1] + c[2] * V[2])) * s);
  pd.order_grid = G;
}

SparseMaskParams make_mask_params(ovr_hip_renderer* r, int frame_index, int32_t* out_xy)
{
  SparseMaskParams m{};
  const FocusP& f = r->focus.current;
  m.noise = r->d_noise;
  m.noise_xy = r->noise_xy;
  m.width = r->fbsize.current.w;
  m.height = r->fbsize.current.h;
  m.frame_index = frame_index;
  m.mean_x = f.cx;
  m.mean_y = f.cy;
  m.sigma_rcp2 = 1.f / (f.scale * f.scale); // generate_mask.cu:90
  m.base_noise = f.base_noise;
  m.out_xy = out_xy;
  m.block_counts = r->d_block_counts;
  m.count = r->d_sparse_count;
  return m;
}

// Screen-space bounding rectangle (pixels, aligned outwards to 8, two pixels of margin for the sub-pixel jitter) of the volume's box
// under the committed camera: a ray outside it misses the box and its pixel is exactly 0 in every layer (background 0, alpha 0,
// shaders_raymarching.cu:260-321) - in any mode: accumulation adds 0, sparse sampling and image shards leave it cleared.  The whole
// frame when a corner of the box lies at or behind the camera plane.  Under the orthographic camera a corner projects without the division by its
// distance - 0.5 + (p . h) / hh - and the rectangle is always valid: what lies outside the silhouette misses (primary_box_test), also on an axis view.
static void nonzero_rect(const ovr_hip_renderer* r, int rect[4])
{
  const int W = r->fbsize.current.w, H = r->fbsize.current.h;
  rect[0] = 0; rect[1] = 0; rect[2] = W; rect[3] = H;
  if (!r->have_volume || W <= 0 || H <= 0) return;
  const RayMarchParams& P = r->P;
  const double d[3] = { P.cam_dir.x, P.cam_dir.y, P.cam_dir.z }, h[3] = { P.cam_hor.x, P.cam_hor.y, P.cam_hor.z }, v[3] = { P.cam_ver.x, P.cam_ver.y, P.cam_ver.z };
  const double hh = h[0] * h[0] + h[1] * h[1] + h[2] * h[2], vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  if (!(hh > 0.0) || !(vv > 0.0)) return;
  const double inv[3] = { P.inv_scale.x, P.inv_scale.y, P.inv_scale.z }, wp[3] = { P.wto_p.x, P.wto_p.y, P.wto_p.z }, from[3] = { P.cam_pos.x, P.cam_pos.y, P.cam_pos.z };
  double sx0 = 1e30, sx1 = -1e30, sy0 = 1e30, sy1 = -1e30;
  for (int c = 0; c < 8; ++c) {
    double p[3];
    for (int k = 0; k < 3; ++k) p[k] = (((c >> k) & 1 ? 1.0 : 0.0) - wp[k]) / inv[k] - from[k]; // object corner -> world, relative to the eye
    const double a = P.cam_orthographic ? 1.0 : p[0] * d[0] + p[1] * d[1] + p[2] * d[2];
    if (!(a > 1e-6 * (std::fabs(p[0]) + std::fabs(p[1]) + std::fabs(p[2]) + 1e-30))) return; // at or behind the camera plane: whole frame
    const double sx = 0.5 + (p[0] * h[0] + p[1] * h[1] + p[2] * h[2]) / (hh * a), sy = 0.5 + (p[0] * v[0] + p[1] * v[1] + p[2] * v[2]) / (vv * a);
    sx0 = std::min(sx0, sx); sx1 = std::max(sx1, sx); sy0 = std::min(sy0, sy); sy1 = std::max(sy1, sy);
  }
  auto lo = [](double s, int n) { const double q = std::floor(s * n) - 2.0; return (int)std::min<double>(std::max<double>(q, 0.0), n) & ~7; };
  auto hi = [](double s, int n) { const double q = std::ceil(s * n) + 2.0; return std::min(((int)std::min<double>(std::max<double>(q, 0.0), n) + 7) & ~7, n); };
  rect[0] = lo(sx0, W); rect[2] = hi(sx1, W); rect[1] = lo(sy0, H); rect[3] = hi(sy1, H);
  if (rect[2] <= rect[0] || rect[3] <= rect[1]) { rect[0] = rect[1] = rect[2] = rect[3] = 0; } // the box is off screen: nothing to refresh
}

// device layer -> pinned host mirror, only where a pixel can differ from 0 now or could when the mirror was last refreshed
int refresh_mirror(ovr_hip_renderer* r, float* host, const float* dev, int channels, const int dev_rect[4], int last[4], hipStream_t st)
{
  const int W = r->fbsize.current.w;
  // what the DEVICE set holds is the frame of the camera it was last rendered with - renderapp commits the next camera before it maps
  // the previous frame (main_app.cpp:244-263) - so the rectangle is the one recorded at render time, not the committed camera's
  int now[4] = { dev_rect[0], dev_rect[1], dev_rect[2], dev_rect[3] };
  static const bool whole = getenv("OVR_HIP_MAP_WHOLE_FRAME") != nullptr; // measurements: the uncropped copy
  if (whole) { now[0] = 0; now[1] = 0; now[2] = W; now[3] = r->fbsize.current.h; }
  int u[4] = { now[0], now[1], now[2], now[3] };
  if (last[2] > last[0] && last[3] > last[1]) {
    if (u[2] <= u[0] || u[3] <= u[1]) { u[0] = last[0]; u[1] = last[1]; u[2] = last[2]; u[3] = last[3]; }
    else { u[0] = std::min(u[0], last[0]); u[1] = std::min(u[1], last[1]); u[2] = std::max(u[2], last[2]); u[3] = std::max(u[3], last[3]); }
  }
  if (u[2] > u[0] && u[3] > u[1]) {
    const size_t pitch = (size_t)W * channels * sizeof(float), off = ((size_t)u[1] * W + u[0]) * channels;
    HIP_TRY(hipMemcpy2DAsync(host + off, pitch, dev + off, pitch, (size_t)(u[2] - u[0]) * channels * sizeof(float), (size_t)(u[3] - u[1]), hipMemcpyDeviceToHost, st));
  }
  for (int k = 0; k < 4; ++k) last[k] = now[k];
  return 0;
}

// the 8x8-pixel blocks of the image this renderer draws (all of them, or those holding a pixel of one of its tiles),
// in image order; the device sorts them by ray length (launch_schedule) before the next frame
static int build_schedule_list(ovr_hip_renderer* r)
{
  const int W = r->fbsize.current.w, H = r->fbsize.current.h;
  const ShardP& s = r->shard.current;
  const int bw = (W + 7) / 8, bh = (H + 7) / 8;
  if (bw > 0xffff || bh > 0xffff) return fail(OVR_HIP_EINVAL, "[hip] framebuffer larger than 524280 pixels on a side");
  std::vector<unsigned int> list;
  list.reserve((size_t)bw * bh / (size_t)std::max(1, s.world) + 64);
  // listed supertile by supertile (4x4 blocks = 32x32 pixels, row-major inside): 16 consecutive entries are a compact square,
  // which the schedule kernel keeps together on one XCD
  const int sw = (bw + 3) / 4, sh = (bh + 3) / 4;
  // order of the supertiles: row-major (0, default) or along a Z curve (OVR_HIP_SCHED_ORDER=morton, round 5 experiment for C4: the blocks of one
  // ray-length class form a ring around the volume's silhouette - in row-major order consecutive entries of a class alternate between the ring's left and
  // right side, on the Z curve they are 2-D patches: do workgroups that run at the same time then share DRAM pages?)
  static const bool morton = getenv("OVR_HIP_SCHED_ORDER") && std::string(getenv("OVR_HIP_SCHED_ORDER")) == "morton";
  std::vector<std::pair<unsigned int, unsigned int>> order; // (key, sx | sy << 16)
  order.reserve((size_t)sw * sh);
  auto spread = [](unsigned int v) { v &= 0xffffu; v = (v | (v << 8)) & 0x00ff00ffu; v = (v | (v << 4)) & 0x0f0f0f0fu; v = (v | (v << 2)) & 0x33333333u; return (v | (v << 1)) & 0x55555555u; };
  for (int sy = 0; sy < sh; ++sy)
    for (int sx = 0; sx < sw; ++sx) order.push_back({ morton ? (spread((unsigned int)sx) | (spread((unsigned int)sy) << 1)) : (unsigned int)(sy * sw + sx), (unsigned int)sx | ((unsigned int)sy << 16) });
  if (morton) std::sort(order.begin(), order.end());
  for (const auto& o : order) {
      const int sx = (int)(o.second & 0xffffu), sy = (int)(o.second >> 16);
      for (int k = 0; k < 16; ++k) {
        const int bx = sx * 4 + (k & 3), by = sy * 4 + (k >> 2);
        if (bx >= bw || by >= bh) continue;
        bool mine = s.world <= 1;
        if (!mine) {
          const int tx0 = (bx * 8) / s.tw, tx1 = std::min(bx * 8 + 7, W - 1) / s.tw;
          const int ty0 = (by * 8) / s.th, ty1 = std::min(by * 8 + 7, H - 1) / s.th;
          for (int ty = ty0; ty <= ty1 && !mine; ++ty)
            for (int tx = tx0; tx <= tx1 && !mine; ++tx) mine = ((tx + ty) % s.world) == s.rank;
        }
        if (mine) list.push_back((unsigned int)bx | ((unsigned int)by << 16));
      }
  }
  if (r->sched.d_src) HIP_TRY(hipFree(r->sched.d_src));
  if (r->sched.d_sorted) HIP_TRY(hipFree(r->sched.d_sorted));
  r->sched.d_src = r->sched.d_sorted = nullptr;
  r->sched.n = (unsigned int)list.size();
  if (!list.empty()) {
    HIP_TRY(hipMalloc((void**)&r->sched.d_src, list.size() * sizeof(unsigned int)));
    HIP_TRY(hipMalloc((void**)&r->sched.d_sorted, (list.size() + schedule_workspace_elems((unsigned int)list.size())) * sizeof(unsigned int))); // + the sort's histograms
    HIP_TRY(hipMemcpy(r->sched.d_src, list.data(), list.size() * sizeof(unsigned int), hipMemcpyHostToDevice));
  }
  r->sched.list_dirty = false;
  r->sched.dirty = true;
  return 0;
}

static int launch_frame(ovr_hip_renderer* r);

// what the steps of one enqueue_frame share
struct FrameSetup {
  hipStream_t st;
  size_t n;         // pixels of the framebuffer
  bool accumulate, sparse;
  bool recon_on;    // pull-push reconstruction: acts on sparse frames of a single renderer that owns the whole image
  bool conv_on;     // convergence estimate / adaptive refinement: defined while frames accumulate and every pixel is sampled
  bool use_skip;    // the frame runs the skipping kernels
};

// step 1, accumulation reset: what a frame must find cleared (device_impl.cpp:226-239)
static int reset_accumulation(ovr_hip_renderer* r, const FrameSetup& f)
{
  hipStream_t st = f.st;
  const size_t n = f.n;
  if (f.accumulate) { // device_impl.cpp:226-233
    if (r->fb_reset) {
      for (int i = 0; i < 2; ++i) {
        // (the set this frame renders into needs no memset when the frame writes every pixel of it: dense sampling, the whole image - launched
        // blocks write their pixels, the others are cleared by launch_clear_blocks; 2 x 7 us per camera change of an accumulating session)
        if (i == r->cur && !f.sparse && r->shard.current.world <= 1) continue;
        // the other set is cleared on ITS stream (whatever touches it next - a frame after a swap, a mapframe - is enqueued there): the memsets
        // run beside this frame's schedule kernels instead of in front of them
        hipStream_t si = (r->use_user_stream || i == r->cur) ? st : r->own_stream[i];
        HIP_TRY(hipMemsetAsync(r->d_rgba[i], 0, n * 4 * sizeof(float), si));
        HIP_TRY(hipMemsetAsync(r->d_grad[i], 0, n * 3 * sizeof(float), si));
      }
      // the reference leaves the accumulation buffer as it is (device_impl.cpp:229-230 are commented out), which is
      // only sound because frame 1 overwrites it; sparse frames do not overwrite every pixel, so it is cleared here
      if (f.sparse) HIP_TRY(hipMemsetAsync(r->d_accum, 0, n * 4 * sizeof(float), st));
      if (f.recon_on) { // N and G start over with A
        HIP_TRY(hipMemsetAsync(r->recon.d_count, 0, std::max<size_t>(n, 1) * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(r->recon.d_grad, 0, std::max<size_t>(n, 1) * 3 * sizeof(float), st));
      }
      r->fb_reset = false;
      r->frame_index = 0;
    }
  }
  else if (f.sparse) { // device_impl.cpp:234-239
    for (int i = 0; i < 2; ++i) {
      HIP_TRY(hipMemsetAsync(r->d_rgba[i], 0, n * 4 * sizeof(float), st));
      HIP_TRY(hipMemsetAsync(r->d_grad[i], 0, n * 3 * sizeof(float), st));
    }
    if (f.recon_on) HIP_TRY(hipMemsetAsync(r->recon.d_count, 0, std::max<size_t>(n, 1) * sizeof(float), st)); // N is this frame's list alone
  }
  r->frame_index++;
  return 0;
}

// step 2, RayMarchParams: the frame's target and its sampling
static void fill_target_params(ovr_hip_renderer* r, const FrameSetup& f)
{
  RayMarchParams& P = r->P;
  P.rgba = r->d_rgba[r->cur];
  nonzero_rect(r, r->d_rect[r->cur]); // what mapframe(HOST) will have to copy of this set (the committed camera is the one this frame renders)
  // an image shard leaves the tiles of the other ranks as they are - whatever an earlier, unsharded frame put there, also outside the box's
  // rectangle: such a set is mapped whole (found by tests/fuzz_states.py, seeds 61 / 62).  (A group leader's set is complete after every
  // frame: its rectangle holds)
  if (r->shard.current.world > 1 && r->group.members.size() <= 1) r->map_whole_set(r->cur);
  if (f.recon_on) r->map_whole_set(r->cur); // a filled frame is not 0 outside the box's rectangle: the set is mapped whole
  r->recon.frame = f.recon_on;
  r->frame_set = r->cur;
  P.grad = r->d_grad[r->cur];
  P.accum = r->d_accum;
  P.width = r->fbsize.current.w;
  P.height = r->fbsize.current.h;
  P.frame_index = r->frame_index;
  P.accumulate = f.accumulate ? 1 : 0;
  P.spp = r->spp.current;
  P.shading = r->shading.current;
  P.step = 1.f / r->rate.current; // volume.cpp:176
  P.base = 1.f;                   // volume.h:125
  P.shadow_stride = (P.step * 10.f) * P.step; // shaders_raymarching.cu:221 then :64
  const float ex = r->spacing[0] * r->vd.nx, ey = r->spacing[1] * r->vd.ny, ez = r->spacing[2] * r->vd.nz;
  P.long_ray_steps = std::sqrt(ex * ex + ey * ey + ez * ez) / P.step;
}

// step 3, layout choice: the layout rule (policy::layout_rule) or the forced layout, then the tuner's second stage (policy::Tuner): the layout /
// pipeline under test, or the measured winner
static void choose_layout(ovr_hip_renderer* r, hipStream_t st)
{
  RayMarchParams& P = r->P;
  int choice = r->layout_choice.current;
  if (choice < 0) {
    const float dir[3] = { P.cam_dir.x, P.cam_dir.y, P.cam_dir.z }, inv_scale[3] = { P.inv_scale.x, P.inv_scale.y, P.inv_scale.z };
    choice = policy::layout_rule(dir, inv_scale);
  }
  const bool tune_l = r->layout_choice.current < 0, tune_p = r->pipeline.current == 0;
  const bool may_wait = !tune_l; // a forced layout is what the frame reads, even if the replica has to be built first
  if (choice < 0 || choice >= kLayouts || r->replica_state[choice] == 0) choice = LAYOUT_GENERAL;
  bool building = false;
  if (r->tune.on && (tune_l || tune_p) && r->tune.state == 1) { // probing: the candidate's replica, and is anything being built?
    int states[kLayouts];
    for (int k = 0; k < kLayouts; ++k) states[k] = r->replica_state[k];
    const int wanted = r->tune.probe_build(tune_l, states);
    if (wanted >= 0) (void)start_replica_build(r, wanted, nullptr);
    building = poll_replica_builds(r) > 0;
    (void)hipGetLastError();
  }
  choice = r->tune.before_frame(choice, tune_l, tune_p, building);
  choice = resolve_layout(r, choice, may_wait, st);
  const float vs = P.vol.value_scale, vm = P.vol.value_min_clamp;
  P.vol = r->vd_replica[choice];
  P.vol.value_scale = vs;
  P.vol.value_min_clamp = vm;
  r->stats.layout = choice;
}

// step 3 of a projection frame (ovr_hip_set_projection): the general layout, whatever the layout choice - the tuner is not consulted
static void bind_general_layout(ovr_hip_renderer* r)
{
  RayMarchParams& P = r->P;
  const float vs = P.vol.value_scale, vm = P.vol.value_min_clamp;
  P.vol = r->vd_replica[LAYOUT_GENERAL];
  P.vol.value_scale = vs;
  P.vol.value_min_clamp = vm;
  r->stats.layout = LAYOUT_GENERAL;
  r->tune.frame = -1; // nothing the layout / pipeline tuner could time
}

const float* projection_ranges(const ovr_hip_renderer* r) { return r->have_volume && r->mc_ranges_valid ? r->d_mc_minmax : nullptr; }

void fill_isosurface_params(const ovr_hip_renderer* r, RayMarchParams& q)
{
  const IsoP& p = r->isosurfaces.current;
  q.iso_n = p.n;
  for (int k = 0; k < OVR_HIP_MAX_ISOVALUES; ++k) q.iso_values[k] = k < p.n ? p.v[k] : 0.f;
  for (int k = 0; k < OVR_HIP_MAX_ISOVALUES; ++k) q.iso_opacities[k] = k < p.n ? p.a[k] : 1.f;
  q.iso_translucent = p.translucent() ? 1 : 0;
  const AoP& ao = r->ambient_occlusion.current; // (the known-answer entries and the lattice's build clear K: launch_ray_query, launch_shadow_cache)
  q.ao_samples = r->d_ao_dirs ? ao.samples : 0;
  q.ao_distance = ao.distance;
  q.ao_dirs = r->d_ao_dirs;
  // the context is kept while no isovalue is committed and takes effect when n > 0 (under committed slices it is bound and not read: committed_frame, launch_plan.hpp)
  const IsoContextP& c = r->isosurface_context.current;
  q.iso_context = (p.n > 0 && c.mode == OVR_HIP_ISO_CONTEXT_VOLUME) ? 1 : 0;
  q.iso_context_scale = c.scale;
}
void fill_slice_params(const ovr_hip_renderer* r, RayMarchParams& q)
{
  const SliceP& p = r->slices.current;
  q.slice_n = p.n;
  for (int k = 0; k < OVR_HIP_MAX_SLICES; ++k) {
    const bool on = k < p.n;
    for (int a = 0; a < 3; ++a) q.slice_plane[k][a] = on ? p.normal[k][a] : 0.f;
    q.slice_plane[k][3] = on ? p.c[k] : 0.f;
    q.slice_half[k] = on ? 0.5f * p.thickness[k] : 0.f;
    q.slice_mode[k] = on && p.thickness[k] > 0.f ? p.mode[k] : 0; // 0: a plane
  }
  // the context is kept while no slice is committed and takes effect when n > 0
  const SliceContextP& c = r->slice_context.current;
  q.slice_context = (p.n > 0 && c.mode == OVR_HIP_SLICE_CONTEXT_FRONT) ? 1 : 0;
  q.slice_context_scale = c.scale;
}
bool preintegrated_frame(const ovr_hip_renderer* r)
{
  return committed_frame(r) == CommittedFrame::March && r->shading.current == OVR_HIP_SHADE_NONE && r->preintegration.current.mode == OVR_HIP_PREINTEGRATION_SEGMENTS;
}
bool gradient_opacity_frame(const ovr_hip_renderer* r)
{
  return gradient_opacity_active(r->gradient_opacity.current.mode, committed_frame(r) == CommittedFrame::March, r->shading.current, preintegrated_frame(r));
}
void fill_gradient_opacity_params(const ovr_hip_renderer* r, RayMarchParams& q, bool on)
{
  const GradientOpacityState& g = r->gradient_opacity.current;
  q.gradient_opacity = on ? 1 : 0;
  q.gradop_lo = g.lo;
  q.gradop_inv_ramp = g.inv_ramp;
}
bool max_depth_frame(const ovr_hip_renderer* r)
{
  const MaxDepthState& m = r->max_depth.current;
  return max_depth_active(m.on && r->d_max_depth != nullptr, committed_frame(r) == CommittedFrame::March, r->shading.current, preintegrated_frame(r), gradient_opacity_frame(r),
                          max_depth_size_matches(m, r->fbsize.current.w, r->fbsize.current.h));
}
bool depth_output_frame(const ovr_hip_renderer* r)
{
  return depth_output_active(r->depth_output.current.mode == kDepthOutputOn, committed_frame(r) == CommittedFrame::March, r->shading.current, preintegrated_frame(r), gradient_opacity_frame(r));
}
int bind_preintegration(ovr_hip_renderer* r, RayMarchParams& q)
{
  q.preintegrated = 1;
  q.preint_m1 = 0;
  q.preint_nodes = nullptr;
  const LaunchPlan pl = plan_raymarch(q);
  if (pl.error || !pl.preintegrated.on || !r->h_tf) return 0;
  const int s = pl.preintegrated.subdivision;
  if (r->preint_generation != r->tf_generation || r->preint_subdivision != s || !r->d_preint_nodes) {
    // (h_tf is rewritten by upload_tfn alone, which raises the generation: between commits it holds the committed tables)
    const int m = build_preintegration_nodes(r->h_tf, r->n_color, r->h_tf + (size_t)r->n_color * 4, r->n_alpha, s, r->preint_table);
    if (m != pl.preintegrated.nodes) return fail(OVR_HIP_EINVAL, "[hip] pre-integration: the node table could not be built");
    if (r->preint_capacity < r->preint_table.size()) {
      HIP_TRY(hipDeviceSynchronize()); // nothing may still read the old table
      if (r->d_preint_nodes) HIP_TRY(hipFree(r->d_preint_nodes));
      r->d_preint_nodes = nullptr; r->preint_capacity = 0;
      HIP_TRY(hipMalloc((void**)&r->d_preint_nodes, r->preint_table.size() * sizeof(float)));
      r->preint_capacity = r->preint_table.size();
    }
    // stream-ordered behind the frames that read the old table; the vector is pageable, so the call returns once it has been staged
    HIP_TRY(hipMemcpyAsync(r->d_preint_nodes, r->preint_table.data(), r->preint_table.size() * sizeof(float), hipMemcpyHostToDevice, r->stream()));
    HIP_TRY(hipStreamSynchronize(r->stream()));
    r->preint_nodes = m;
    r->preint_subdivision = s;
    r->preint_generation = r->tf_generation;
  }
  q.preint_m1 = r->preint_nodes - 1;
  q.preint_nodes = r->d_preint_nodes;
  return 0;
}
// a frame drawn by one kernel in the march's place, from the general layout: a projection, the isosurfaces, the slices, the pre-integrated, the gradient-opacity, the depth-limited or the depth-output march
static bool in_place_frame(const RayMarchParams& P)
{
  return ovrhip::committed_frame(P.slice_n, P.iso_n, P.projection) != CommittedFrame::March || P.preintegrated != 0 || P.gradient_opacity != 0 || P.max_depth != nullptr || P.depth_tau > 0.f;
}

// step 2, continued: tables, shard, jitter, counters
static int fill_table_params(ovr_hip_renderer* r)
{
  RayMarchParams& P = r->P;
  P.tf_color = r->d_tf_color;
  P.tf_alpha = r->d_tf_alpha;
  P.n_color = r->n_color;
  P.n_alpha = r->n_alpha;
  P.rank = r->shard.current.rank;
  P.world = r->shard.current.world;
  P.tile_w = r->shard.current.tw;
  P.tile_h = r->shard.current.th;
  P.lds_staging = r->lds_staging.current;
  P.lds_brick_offset = 0;
  P.jitter_mode = r->jitter.current;
  P.jitter_noise = r->d_noise;
  P.jitter_xy = r->noise_xy;
  if (P.jitter_mode == 1 && !r->d_noise)
    return fail(OVR_HIP_ESTATE, "[hip] blue-noise pixel jitter enabled but no noise tile was set (ovr_hip_set_noise_tile)");
  P.counters = r->d_counters;
  P.majorant = nullptr;
  P.occupancy = nullptr;
  P.occupancy_fine = nullptr;
  P.projection = r->projection.current;
  P.mc_ranges = nullptr;
  fill_isosurface_params(r, P);
  fill_slice_params(r, P);
  P.preintegrated = preintegrated_frame(r) ? 1 : 0;
  P.preint_m1 = 0;
  P.preint_nodes = nullptr;
  fill_gradient_opacity_params(r, P, gradient_opacity_frame(r));
  P.max_depth = max_depth_frame(r) ? r->d_max_depth : nullptr; // (the image of the committed framebuffer's size: the kernel indexes it as it indexes the frame)
  P.depth_tau = depth_output_frame(r) ? r->depth_output.current.threshold : 0.f; // (> 0 in mode ON: the depth frame, which applies P.max_depth where it is bound)
  return 0;
}

// step 4, skipping: the skipping kernels if they are enabled and pay (policy::Skip), the shade grid that goes with them, and what every frame
// starts from
static int choose_skipping(ovr_hip_renderer* r, FrameSetup& f)
{
  RayMarchParams& P = r->P;
  // a projection or isosurface frame skips by the macrocells' value ranges, which need no majorants: the adaptive-skipping probe is not consulted
  if (in_place_frame(P)) {
    f.use_skip = false;
    if (r->skipping.current != 0) P.mc_ranges = projection_ranges(r);
  }
  else f.use_skip = r->skip.before_frame(r->skipping.current != 0, r->mc_majorant_valid);
  if (f.use_skip) {
    if (int e = update_macrocells(r, f.st)) return e;
    P.majorant = r->d_mc_majorant;
    P.occupancy = r->d_mc_occupancy;
    P.occupancy_fine = r->d_mc_fine;
  }
  P.shade_blocks = policy::shade_blocks(f.use_skip, r->stats.pool_chunks);
  P.block_counters = r->d_block_counters;
  P.trace = r->d_trace;
  P.sparse_xy = nullptr;
  P.sparse_count = nullptr;
  P.sparse_hint_pixels = 0;
  P.schedule = nullptr;
  P.n_schedule = 0;
  P.n_blocks_owned = 0;
  r->sched.frame_empty_pixels = 0;
  r->sched.frame_empty_rays = 0;
  return 0;
}

// step 5, schedule (dense frames): the launch list of the march's workgroups, sorted again when the camera or the volume's box changed, and the
// blocks that are not launched cleared
static int schedule_blocks(ovr_hip_renderer* r, const FrameSetup& f)
{
  RayMarchParams& P = r->P;
  hipStream_t st = f.st;
  ScheduleState& s = r->sched;
  if (s.list_dirty)
    if (int e = build_schedule_list(r)) return e;
  static const bool unsorted = getenv("OVR_HIP_SCHED_SORT") && atoi(getenv("OVR_HIP_SCHED_SORT")) == 0; // experiment: image (supertile) order
  static const bool skip_blocks = !(getenv("OVR_HIP_EMPTY_BLOCKS") && atoi(getenv("OVR_HIP_EMPTY_BLOCKS")) == 0); // 0: launch every block (measurements)
  const int exact = policy::schedule_exact(skip_blocks, unsorted, P.spp, P.jitter_mode);
  if (s.dirty || exact != s.exact) {
    if (!s.h_info) HIP_TRY(hipHostMalloc((void**)&s.h_info, 2 * sizeof(unsigned int), hipHostMallocDefault)); // pinned: the scatter kernel writes it
    HIP_TRY(launch_schedule(P, s.d_src, s.n, s.d_sorted, s.d_sorted + s.n, exact, s.h_info, st));
    s.n_work = s.n;
    s.empty_pixels = 0;
    if (exact && s.n > 0) { // how many entries need a workgroup: two words from the device, once per camera / volume / size change
      // (in a device group every member waits on its own thread, side by side - round 5)
      HIP_TRY(hipStreamSynchronize(st));
      s.n_work = std::min(s.h_info[0], s.n);
      s.empty_pixels = s.h_info[1];
    }
    s.dirty = false;
    s.exact = exact;
    s.clear_gen++;
  }
  P.schedule = unsorted ? s.d_src : s.d_sorted;
  P.n_schedule = s.n_work;
  P.n_blocks_owned = s.n;
  s.frame_empty_pixels = s.empty_pixels;
  s.frame_empty_rays = (unsigned long long)s.empty_pixels * (unsigned long long)std::max(P.spp, 1); // every sample of a pixel is a ray
  if (s.n_work < s.n) {
    const bool first_accumulated = f.accumulate && r->frame_index == 1;
    if (s.set_clear_gen[r->cur] != s.clear_gen || first_accumulated) {
      HIP_TRY(launch_clear_blocks(P, s.d_sorted + s.n_work, s.n - s.n_work, first_accumulated ? 1 : 0, st));
      s.set_clear_gen[r->cur] = s.clear_gen;
    }
  }
  return 0;
}

// step 6, convergence: a new accumulation starts the estimate over; an adaptive frame marches the active blocks only.  With every block
// retired the frame is the resolve alone (conv.resolve_only): the caller launches it as it is
static int prepare_convergence(ovr_hip_renderer* r, const FrameSetup& f)
{
  RayMarchParams& P = r->P;
  hipStream_t st = f.st;
  ConvergenceState& c = r->conv;
  c.frame = c.resolve_only = false;
  if (!f.conv_on) { c.valid = false; return 0; }
  const bool adaptive = r->convergence.current.mode == OVR_HIP_CONVERGENCE_ADAPTIVE;
  if (int e = ensure_convergence(r, true)) return e;
  if (r->frame_index == 1) { // a new accumulation: no estimate yet, every block is active again (sched.d_sorted still holds them all, sorted)
    HIP_TRY(hipMemsetAsync(c.d_error, 0, std::max<size_t>(c.blocks, 1) * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(c.d_frames, 0, std::max<size_t>(c.blocks, 1) * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(c.d_words, 0, 4 * sizeof(unsigned int), st));
    // an image shard writes its own tiles only: what an earlier shard or an unsharded accumulation left in the others is not H
    if (r->shard.current.world > 1) HIP_TRY(hipMemsetAsync(c.d_accum_half, 0, std::max<size_t>(f.n, 1) * 4 * sizeof(float), st));
    c.valid = false;
    c.error = 0.f;
    c.frames = 0;
    c.active = r->sched.n_work;
    c.retired = 0;
  }
  P.conv_asked = c.d_words + 2;
  c.sorted = P.schedule;
  c.frame = (r->frame_index & 1) == 0;
  if (adaptive && c.retired > 0) {
    P.schedule = c.d_lists; // the active entries, still longest rays first
    P.n_schedule = c.active;
    if (c.active == 0) { // every block is retired: the frame is the resolve alone
      c.resolve_only = true;
      c.frame = false;
      r->tune.frame = -1;      // nothing the layout / pipeline tuner could time
      P.pool = PoolDesc{};
    }
  }
  return 0;
}

// step 7, sparse mask: the frame's own pixel list (createSparseSamples, device_impl.cpp:304-342)
static int launch_frame_mask(ovr_hip_renderer* r, const FrameSetup& f)
{
  RayMarchParams& P = r->P;
  if (!r->d_noise) return fail(OVR_HIP_ESTATE, "[hip] sparse sampling enabled but no noise tile was set (ovr_hip_set_noise_tile)");
  if (int e = ensure_sparse_buffers(r)) return e;
  SparseMaskParams mp = make_mask_params(r, r->frame_index, r->d_sparse_xy);
  mp.tile_major = 1; // the frame's own list: 4x4-pixel blocks per wave where the mask is dense (the kept pixels are the same)
  HIP_TRY(launch_sparse_mask(mp, f.st));
  P.sparse_xy = r->d_sparse_xy;
  P.sparse_count = r->d_sparse_count;
  P.sparse_hint_pixels = r->sparse_prev_pixels;
  if (f.recon_on) P.conv_asked = r->recon.d_words; // words[0]: an attempt that overflowed the request pool is not counted and not filled
  return 0;
}

// step 8, pool - the shading pipeline: pooled (march -> shade -> composite) when it applies, else in place
static int prepare_pool(ovr_hip_renderer* r, const FrameSetup& f)
{
  RayMarchParams& P = r->P;
  const size_t n = f.n;
  const bool want_pool = !in_place_frame(P) && r->auto_pipe.want_pool(P.shading, r->pipeline.current, r->tune.measured_pipeline()); // (a projection: in place)
  P.pool = PoolDesc{};
  if (want_pool) {
    size_t guess = policy::pool_first_guess(n, r->pool_tiles); // grown after an overflow (resolve_pool)
    if (const char* pc = getenv("OVR_HIP_POOL_CHUNKS")) guess = std::max<size_t>(8, (size_t)atoll(pc)); // diagnostic: force the overflow path
    if (int e = ensure_pool(r, std::max<size_t>(guess, r->pool.capacity))) return e;
    if (!r->pool.ctrl) {
      r->pool.ctrl = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(r->d_counters) + 128); // every sub-pool counter on a 128-byte line of its own
      HIP_TRY(hipMalloc((void**)&r->pool.shade_counters, pool_shade_blocks() * 2 * sizeof(unsigned int)));
    }
    P.pool = r->pool;
    shade_order_params(r, P.pool);
    if (P.spp > 1 && !r->d_spp_rgba) {
      HIP_TRY(hipMalloc((void**)&r->d_spp_rgba, std::max<size_t>(n, 1) * 4 * sizeof(float)));
      HIP_TRY(hipMalloc((void**)&r->d_spp_grad, std::max<size_t>(n, 1) * 3 * sizeof(float)));
    }
  }
  P.spp_index = 0;
  P.spp_sum_rgba = r->d_spp_rgba;
  P.spp_sum_grad = r->d_spp_grad;
  r->stats.pipeline = want_pool ? 2 : 1;
  return 0;
}

// ---- shadow cache (ovr_hip_set_shadow_cache)
int shadow_lattice_dims(const ovr_hip_renderer* r, int cell, int dims[3])
{
  const int n[3] = { r->vd.nx, r->vd.ny, r->vd.nz };
  long long nodes = 1;
  for (int k = 0; k < 3; ++k) {
    const long long nk = policy::shadow_cache_nodes(n[k], std::max(cell, 1));
    nodes = nodes > 0x7fffffffll / nk ? 0x80000000ll : nodes * nk;
    dims[k] = (int)std::min<long long>(nk, 0x7fffffffll);
  }
  if (nodes > 0x7fffffffll) return fail(OVR_HIP_EINVAL, "[hip] shadow cache: a lattice of more than 2^31 - 1 nodes (take a larger cell)");
  return 0;
}

// what the shadow march reads beyond the committed volume transform, light and clip box, as a frame sets it: the sampling rate's constants, the transfer
// function's tables and the GENERAL layout - always resident, and what ovr_hip_update_volume rewrites
void fill_shadow_params(ovr_hip_renderer* r, RayMarchParams& q)
{
  q.step = 1.f / r->rate.current;
  q.base = 1.f;
  q.shadow_stride = (q.step * 10.f) * q.step;
  q.tf_color = r->d_tf_color; q.tf_alpha = r->d_tf_alpha;
  q.n_color = r->n_color; q.n_alpha = r->n_alpha;
  const float vs = q.vol.value_scale, vm = q.vol.value_min_clamp;
  q.vol = r->vd_replica[LAYOUT_GENERAL];
  q.vol.value_scale = vs;
  q.vol.value_min_clamp = vm;
  q.grad = nullptr;
}

// nodes' positions: origin + u * (spacing * extent), the extent of update_volume_params
static void shadow_lattice_frame(const ovr_hip_renderer* r, ShadowBuildArgs& a)
{
  const bool vertex = r->grid_convention.current == OVR_HIP_GRID_VERTEX_CENTRED;
  const int n[3] = { r->vd.nx, r->vd.ny, r->vd.nz };
  for (int k = 0; k < 3; ++k) {
    const float ext = vertex ? (float)(n[k] - 1) : (float)n[k];
    a.sc[k] = r->spacing[k] * ext;
    a.origin[k] = r->origin[k];
  }
}

// binds the lattice the committed mode reads into q (null in mode MARCHED); mode CACHED builds it first when it is stale.  The build runs on st in front
// of whatever follows and is waited for: its time and iterations are the build's own (ovr_hip_get_shadow_cache), never part of a frame's kernel_ms
int ensure_shadow_cache(ovr_hip_renderer* r, RayMarchParams& q, hipStream_t st)
{
  ShadowCacheState& c = r->shadow_cache;
  const ShadowP& sp = r->shadow.current;
  q.shadow_lattice = nullptr;
  q.shadow_n1[0] = q.shadow_n1[1] = q.shadow_n1[2] = 1;
  if (sp.mode == OVR_HIP_SHADOWS_MARCHED) return 0;
  if (sp.mode == OVR_HIP_SHADOWS_SUPPLIED) {
    if (!c.d_supplied) return fail(OVR_HIP_ESTATE, "[hip] shadow cache: mode SUPPLIED without values (ovr_hip_set_shadow_cache_values)");
    q.shadow_lattice = c.d_supplied;
    for (int k = 0; k < 3; ++k) q.shadow_n1[k] = c.supplied_dims[k] - 1;
    return 0;
  }
  if (!c.built_valid) {
    if (!r->have_volume || !r->have_tfn) return fail(OVR_HIP_ESTATE, "[hip] shadow cache: the build needs a volume and a transfer function");
    int dims[3];
    if (int e = shadow_lattice_dims(r, sp.cell, dims)) return e;
    const size_t nodes = (size_t)dims[0] * dims[1] * dims[2];
    if (nodes > c.built_cap) { // the new buffer first: a failed allocation leaves the old one in place
      float* d = nullptr;
      if (hipMalloc((void**)&d, nodes * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OVR_HIP_EDEVICE, "[hip] shadow cache: the lattice of " + std::to_string(nodes) + " nodes could not be allocated");
      }
      if (c.d_built) HIP_TRY(hipFree(c.d_built));
      c.d_built = d;
      c.built_cap = nodes;
    }
    if (!c.d_iterations) HIP_TRY(hipMalloc((void**)&c.d_iterations, sizeof(unsigned long long)));
    for (int i = 0; i < 2; ++i)
      if (!c.ev[i]) HIP_TRY(hipEventCreate(&c.ev[i]));
    RayMarchParams b = r->P;
    fill_shadow_params(r, b);
    ShadowBuildArgs a{};
    a.out = c.d_built;
    a.n = (long long)nodes;
    a.nx = dims[0]; a.ny = dims[1]; a.nz = dims[2];
    shadow_lattice_frame(r, a);
    a.iterations = c.d_iterations;
    if (r->tf_copy_pending) { HIP_TRY(hipStreamWaitEvent(st, r->ev_tf, 0)); r->tf_copy_pending = false; }
    HIP_TRY(hipMemsetAsync(c.d_iterations, 0, sizeof(unsigned long long), st));
    HIP_TRY(hipEventRecord(c.ev[0], st));
    HIP_TRY(launch_shadow_cache(b, a, st));
    HIP_TRY(hipEventRecord(c.ev[1], st));
    unsigned long long it = 0;
    HIP_TRY(hipMemcpyAsync(&it, c.d_iterations, sizeof(it), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    for (int k = 0; k < 3; ++k) c.built_dims[k] = dims[k];
    c.built_valid = true;
    c.builds++;
    c.build_samples = it;
    c.build_ms = ms;
  }
  q.shadow_lattice = c.d_built;
  for (int k = 0; k < 3; ++k) q.shadow_n1[k] = c.built_dims[k] - 1;
  return 0;
}

// the nodes' world positions of an nx x ny x nz lattice over the resident volume, as the build kernel forms them (ovr_hip_get_shadow_cache_values)
int shadow_lattice_positions(ovr_hip_renderer* r, const int dims[3], float* d_pos, hipStream_t st)
{
  RayMarchParams b = r->P;
  fill_shadow_params(r, b);
  ShadowBuildArgs a{};
  a.pos_out = d_pos;
  a.n = (long long)dims[0] * dims[1] * dims[2];
  a.nx = dims[0]; a.ny = dims[1]; a.nz = dims[2];
  shadow_lattice_frame(r, a);
  HIP_TRY(launch_shadow_cache(b, a, st));
  return 0;
}

// Impl::render up to and including the launch (device_impl.cpp:199-262); no host synchronisation
int enqueue_frame(ovr_hip_renderer* r)
{
  if (!r->have_volume) return fail(OVR_HIP_ESTATE, "[hip] render() called before a volume was set");
  if (!r->have_tfn) return fail(OVR_HIP_ESTATE, "[hip] render() called before a transfer function was set");
  if (raymarch_lds_bytes(r->n_color, r->n_alpha) == 0)
    return fail(OVR_HIP_EINVAL, "[hip] transfer function too large for LDS staging (colour + alpha tables must fit in 96 KiB)");
  if (r->fbsize.current.w <= 0 || r->fbsize.current.h <= 0) return 0; // device_impl.cpp:216-217
  hipStream_t st = r->stream();
  if (r->use_user_stream) {
    // A frame is not a capturable unit: its first and last events carry timing, the frame after a camera / volume / size change waits for two
    // words from the device, and the host reads the frame's counters when it resolves it - a caller's stream under graph capture is refused, not corrupted
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
      return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_render_async: the caller's stream is capturing a graph - frames cannot be captured (they record timed events and hand "
                                  "counters back to the host); enqueue them on the stream outside the capture");
    (void)hipGetLastError();
  }
  if (r->tf_copy_pending) { HIP_TRY(hipStreamWaitEvent(st, r->ev_tf, 0)); r->tf_copy_pending = false; } // the tables' copy may sit on the other set's stream
  FrameSetup f{};
  f.st = st;
  f.n = r->fb_pixels;
  f.accumulate = r->accumulate.current != 0;
  f.sparse = r->sparse.current != 0;
  f.recon_on = r->reconstruction.current == OVR_HIP_RECONSTRUCT_FILL && f.sparse && r->shard.current.world <= 1 && r->group.members.size() <= 1 && !r->group.leader;
  if (f.recon_on)
    if (int e = ensure_reconstruction(r)) return e;
  if (int e = reset_accumulation(r, f)) return e;
  fill_target_params(r, f);
  if (committed_frame(r) != CommittedFrame::March || preintegrated_frame(r) || gradient_opacity_frame(r) || max_depth_frame(r) || depth_output_frame(r)) bind_general_layout(r);
  else choose_layout(r, st);
  if (int e = fill_table_params(r)) return e;
  if (int e = choose_skipping(r, f)) return e;
  if (r->P.preintegrated)
    if (int e = bind_preintegration(r, r->P)) return e;
  // the shadow cache: a frame with full shading reads the lattice of a mode other than MARCHED (built here, in front of the frame, when it is stale)
  r->P.shadow_lattice = nullptr;
  if (!in_place_frame(r->P) && r->P.shading == OVR_HIP_SHADE_FULL && r->shadow.current.mode != OVR_HIP_SHADOWS_MARCHED)
    if (int e = ensure_shadow_cache(r, r->P, st)) return e;
  f.conv_on = r->convergence.current.mode != OVR_HIP_CONVERGENCE_OFF && f.accumulate && !f.sparse;
  r->P.accum_half = nullptr; // (before launch_clear_blocks: H is cleared with A)
  r->P.conv_asked = nullptr;
  if (f.conv_on) {
    if (int e = ensure_convergence(r, false)) return e;
    r->P.accum_half = r->conv.d_accum_half;
  }
  if (!f.sparse)
    if (int e = schedule_blocks(r, f)) return e;
  if (int e = prepare_convergence(r, f)) return e;
  if (r->conv.resolve_only) return launch_frame(r);
  if (f.sparse)
    if (int e = launch_frame_mask(r, f)) return e;
  if (int e = prepare_pool(r, f)) return e;
  return launch_frame(r);
}

static int launch_frame(ovr_hip_renderer* r)
{
  hipStream_t st = r->stream();
  const bool resolve = r->P.accum_half && r->convergence.current.mode == OVR_HIP_CONVERGENCE_ADAPTIVE && r->conv.retired > 0;
  const int blocks_x = (r->fbsize.current.w + 7) / 8;
  if (r->conv.resolve_only) { // (no march, no counters: the host's copy of them reads 0)
    HIP_TRY(hipEventRecord(r->ev[0], st));
    HIP_TRY(launch_resolve_blocks(r->P, r->conv.d_lists + r->conv.list_cap, r->conv.retired, r->conv.d_frames, r->conv.d_grad_keep, blocks_x, st));
    HIP_TRY(hipEventRecord(r->ev[3], st));
    std::memset(r->h_counters, 0, 8 * sizeof(unsigned long long));
    r->frame_phase_timed = false;
    r->async_pending = true;
    return 0;
  }
  // retired blocks get their pixels from the resolve (disjoint from what the march writes), in whichever set this frame renders into
  if (resolve) HIP_TRY(launch_resolve_blocks(r->P, r->conv.d_lists + r->conv.list_cap, r->conv.retired, r->conv.d_frames, r->conv.d_grad_keep, blocks_x, st));
  // the frame's last reduction kernel writes the counters and the pool's control words into h_counters / h_ctrl itself and zeroes them on the
  // device for the next frame (RayMarchParams::publish): a frame is its kernels, nothing in front of them and nothing behind
  r->P.publish = r->h_counters;
  r->P.reduce_done = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(r->d_counters) + 128 + (size_t)kPoolCtrlWords * sizeof(unsigned int));
  r->P.zero_first = r->frame_words_dirty ? 1 : 0;
  if (r->frame_words_dirty) HIP_TRY(hipMemsetAsync(r->P.reduce_done, 0, sizeof(unsigned int), st));
  if (r->frame_words_dirty && r->pool.order_ws) HIP_TRY(hipMemsetAsync(r->pool.order_ws, 0, (size_t)kOrderWsWords * sizeof(unsigned int), st)); // (a march without its shade kernel)
  r->frame_words_dirty = true; // until the launch below has been enqueued completely
  // the events between the frame's kernels (per-phase times) cost ~16 us a frame - hipEventRecord is not free on either side of the queue; the
  // first and the last one (kernel_ms: what the layout / pipeline tuner compares) stay
  const bool phases = r->phase_timing.load();
  hipEvent_t evs[4] = { r->ev[0], phases ? r->ev[1] : nullptr, phases ? r->ev[2] : nullptr, r->ev[3] };
  r->frame_phase_timed = phases;
  r->plan = plan_raymarch(r->P);
  HIP_TRY(launch_raymarch(r->P, r->plan, st, evs));
  r->frame_words_dirty = false;
  if (r->conv.frame) { // behind the frame's last kernel and its last event: kernel_ms stays the frame's own time
    ConvergenceParams c{};
    c.accum = r->d_accum; c.accum_half = r->conv.d_accum_half; c.grad = r->P.grad; c.grad_keep = r->conv.d_grad_keep;
    c.width = r->P.width; c.height = r->P.height; c.frame_index = r->P.frame_index;
    c.rank = r->P.rank; c.world = r->P.world; c.tile_w = r->P.tile_w; c.tile_h = r->P.tile_h;
    c.blocks_x = blocks_x;
    c.adaptive = r->convergence.current.mode == OVR_HIP_CONVERGENCE_ADAPTIVE ? 1 : 0;
    c.threshold = r->convergence.current.threshold;
    c.sorted = r->conv.sorted; c.n_work = r->sched.n_work;
    c.active = r->P.schedule; c.n_active = r->P.n_schedule;
    c.active_out = r->conv.d_lists; c.retired_out = r->conv.d_lists ? r->conv.d_lists + r->conv.list_cap : nullptr;
    c.counts = r->conv.d_lists ? r->conv.d_lists + 2 * r->conv.list_cap : nullptr;
    c.block_error = r->conv.d_error; c.block_frames = r->conv.d_frames; c.words = r->conv.d_words;
    c.sub_capacity = r->P.pool.reqs ? r->P.pool.sub_capacity : 0xffffffffu;
    c.publish = r->conv.h_publish;
    r->conv.h_publish[3] = 0u; // (finish_frame_one expects this frame's number here)
    HIP_TRY(launch_convergence(c, st));
  }
  if (r->recon.frame) { // behind the frame's last kernel and its last event, like the estimate: kernel_ms stays the frame's own time
    ReconParams& c = r->recon.params;
    c = ReconParams{};
    c.width = r->P.width; c.height = r->P.height;
    (void)recon_plan(c);
    c.rgba = r->P.rgba; c.grad = r->P.grad;
    c.count = r->recon.d_count;
    c.accum = r->P.accumulate ? r->d_accum : nullptr;
    c.grad_sum = r->P.accumulate ? r->recon.d_grad : nullptr;
    c.pyramid = r->recon.d_pyramid;
    c.words = r->recon.d_words;
    c.sub_capacity = r->P.pool.reqs ? r->P.pool.sub_capacity : 0xffffffffu;
    c.publish = r->recon.h_publish;
    c.frame_index = r->P.frame_index;
    r->recon.h_publish[1] = 0u; // (finish_frame_one expects this frame's number here)
    r->recon.timed = phases;
    if (phases) HIP_TRY(hipEventRecord(r->recon.ev[0], st));
    HIP_TRY(launch_recon_scatter(c, r->recon.d_count, r->P.accumulate ? r->recon.d_grad : nullptr, r->P.sparse_xy, r->P.sparse_count, st));
    HIP_TRY(launch_reconstruct(c, st));
    if (phases) HIP_TRY(hipEventRecord(r->recon.ev[1], st));
  }
  r->async_pending = true;
  return 0;
}

// the request pool of the frame that has just ended: an overflowing frame is rendered again with a larger pool
static int resolve_pool(ovr_hip_renderer* r)
{
  if (r->P.pool.reqs) {
    // pool overflow: the march asked for more chunks than the pool holds; nothing was written to the framebuffer.
    // Grow the pool to what the frame needs (+25 %) and render the same frame again.
    // the most chunks any sub-pool was asked for in any generation of the frame
    auto asked = [&]() { return (size_t)r->h_ctrl[32 * (kPoolSubs + 1)]; };
    if (asked() > r->pool.sub_capacity && r->packed_early) r->stats.stale_tiles = 1; // packed before this re-render: the caller must not use them
    for (int attempt = 0; attempt < 4 && asked() > r->pool.sub_capacity; ++attempt) {
      if (int e = ensure_pool(r, policy::pool_grown(asked()))) return e;
      r->P.pool = r->pool;
      shade_order_params(r, r->P.pool);
      if (int e = launch_frame(r)) return e;
      HIP_TRY(hipStreamSynchronize(r->stream()));
    }
    if (asked() > r->pool.sub_capacity) return fail(OVR_HIP_EDEVICE, "[hip] request pool overflow persists after re-sizing");
    size_t used = 0; // chunks reserved by the last generation
    for (int k = 0; k < kPoolSubs; ++k) used += r->h_ctrl[32 * (k + 1)];
    r->stats.pool_chunks = used;
    r->pool_roomy = asked() * 2 <= (size_t)r->pool.sub_capacity;
  }
  else {
    // no pool: this frame is never rendered twice - but it proves nothing about the pool: only a pooled frame of the same
    // configuration does (the automatic pipeline may flip the NEXT frame back to pooled without a commit in between, and
    // ovr_hip_pack_tiles packs right behind a frame only when pool_roomy says it cannot overflow)
    r->stats.pool_chunks = 0;
    r->pool_roomy = false;
  }
  return 0;
}

// the frame's times and counters into ovr_hip_stats
static int read_frame_stats(ovr_hip_renderer* r)
{
  float ms = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, r->ev[0], r->ev[3]));
  if (r->frame_phase_timed) {
    HIP_TRY(hipEventElapsedTime(&m1, r->ev[0], r->ev[1]));
    HIP_TRY(hipEventElapsedTime(&m2, r->ev[1], r->ev[2]));
    HIP_TRY(hipEventElapsedTime(&m3, r->ev[2], r->ev[3]));
  }
  r->stats.kernel_ms = ms;
  r->stats.march_ms = m1;
  r->stats.shade_ms = m2;
  r->stats.composite_ms = m3;
  r->stats.rays = r->h_counters[0] + r->sched.frame_empty_rays;   // (blocks without a hit are not launched: their pixels' rays missed)
  r->stats.samples = r->h_counters[1];
  r->stats.shaded_samples = r->h_counters[2];
  r->stats.shadow_samples = r->h_counters[3];
  r->stats.active_pixels = r->h_counters[4] + r->sched.frame_empty_pixels;
  r->stats.skipped_samples = r->h_counters[5];
  r->stats.skipped_shadow_samples = r->h_counters[6];
  // The reference's box test switches a slab off for a ray whose direction component on that axis is below FLT_MIN (shaders_common.h:162-172,
  // restated): such a ray hits the box wherever its origin lies along that axis - from OUTSIDE the box's silhouette if the origin is
  // outside the slab (an axis-aligned camera's centre row / column; any camera now and then, by one pixel on the line where a component
  // changes sign).  The march counts those hits; a frame that has one - or accumulates onto one - is mapped whole, not by its rectangle.
  if (r->accumulate.current == 0 || r->frame_index <= 1) r->outside_hits = false;
  if (r->h_counters[7] > 0) r->outside_hits = true;
  if (r->outside_hits) r->map_whole_set(r->frame_set);
  r->stats.lds_fallback_taps = r->stats.lds_unstaged_rounds = r->stats.lds_rounds = 0;
  if (r->plan.march.lds_staged) {
    // the unshaded f32 march ran its LDS-staged variant: the two skip counters carried its diagnostics
    r->stats.lds_fallback_taps = r->h_counters[5];
    r->stats.lds_unstaged_rounds = r->h_counters[6];
    r->stats.lds_rounds = r->h_counters[3];
    r->stats.skipped_samples = r->stats.skipped_shadow_samples = r->stats.shadow_samples = 0;
  }
  r->stats.frame_index = r->frame_index;
  r->sparse_prev_pixels = r->P.sparse_xy ? r->stats.active_pixels : 0;
  r->stats.skipping_kernels = r->skip.frame_used ? 1 : 0;
  // a frame of one kernel in the march's place: which twin ran (the adaptive-skipping probe had no say), kept for the kind's getter
  switch (frame_kind(r->plan)) {
  case FrameKind::March: break;
  case FrameKind::PreintegratedMarch: case FrameKind::GradientOpacityMarch: case FrameKind::DepthLimitedMarch: case FrameKind::DepthOutputMarch: r->stats.skipping_kernels = 0; break; // (they fetch every step)
  case FrameKind::Projection: r->stats.skipping_kernels = r->projection_skipped = r->plan.project.skip; break;
  case FrameKind::Isosurface: case FrameKind::IsosurfaceLayers: case FrameKind::IsosurfaceAo: case FrameKind::IsosurfaceContext:
    r->stats.skipping_kernels = r->isosurface_skipped = r->plan.isosurface.skip;
    break;
  case FrameKind::SlicePlane: case FrameKind::SliceWalk: case FrameKind::SliceContext: r->stats.skipping_kernels = r->slices_skipped = r->plan.slices.skip; break;
  }
  r->stats.replicas_building = poll_replica_builds(r);
  (void)hipGetLastError(); // hipErrorNotReady of the query is not an error
  return 0;
}

// what the policies read of the frame that has just ended
static policy::FrameWork frame_work(const ovr_hip_renderer* r)
{
  policy::FrameWork w;
  w.samples = r->stats.samples;
  w.shaded_samples = r->stats.shaded_samples;
  w.shadow_samples = r->stats.shadow_samples;
  w.skipped_samples = r->stats.skipped_samples;
  w.skipped_shadow_samples = r->stats.skipped_shadow_samples;
  w.shading = r->P.shading;
  w.spp = r->P.spp;
  w.layout = r->stats.layout;
  w.pipeline = r->stats.pipeline;
  w.kernel_ms = (float)r->stats.kernel_ms;
  return w;
}

// the layout / pipeline tuner's turn (policy::Tuner): the frame was a candidate, or runs a decision that is being kept
static void tune_after_frame(ovr_hip_renderer* r, const policy::FrameWork& w)
{
  policy::Tuner& t = r->tune;
  r->stats.tuning = t.status();
  bool trace = false;
  if (t.frame >= 0 && t.state < 2) { // a candidate
    static const bool trace_on = getenv("OVR_HIP_TUNE_TRACE") != nullptr;
    trace = trace_on;
    const policy::Tuner::Cand& c = t.cand[t.frame];
    if (trace) fprintf(stderr, "[hip] tune: state %d phase %d candidate %d (layout %d pipeline %d) frame %d: layout %d pipeline %d kernel %.3f ms\n", t.state, t.phase,
                       t.frame, c.layout, c.pipeline, c.frames + 1, r->stats.layout, r->stats.pipeline, w.kernel_ms);
  }
  int states[kLayouts];
  for (int k = 0; k < kLayouts; ++k) states[k] = r->replica_state[k];
  const policy::Tuner::After a = t.after_frame(w, r->layout_choice.current < 0, r->pipeline.current == 0, states);
  for (int k = 1; k < kLayouts; ++k)
    if (a.builds & (1u << k)) (void)start_replica_build(r, k, nullptr); // built while the candidates before it are timed
  if (trace && a.decided) fprintf(stderr, "[hip] tune: decided layout %d pipeline %d (%.3f ms)\n", t.layout, t.pipeline, a.best_ms);
}

// the estimate behind this (even) frame, published by its last kernel
static int read_convergence(ovr_hip_renderer* r)
{
  ConvergenceState& c = r->conv;
  if (c.h_publish[3] != (unsigned int)r->frame_index) return fail(OVR_HIP_EDEVICE, "[hip] the convergence estimate of the frame was not published");
  std::memcpy(&c.error, &c.h_publish[0], sizeof(float));
  c.frames = r->frame_index;
  c.valid = true;
  if (r->convergence.current.mode == OVR_HIP_CONVERGENCE_ADAPTIVE) {
    // the tuner compares kernel times of consecutive frames: candidates timed on different amounts of work are not comparable - it starts over
    if (c.h_publish[1] != c.active) r->tune.work_changed();
    c.active = c.h_publish[1];
    c.retired = c.h_publish[2];
  }
  return 0;
}

// what the reconstruction behind this frame did, published by its last kernel
static int read_reconstruction(ovr_hip_renderer* r)
{
  ReconstructionState& c = r->recon;
  c.info = ovr_hip_reconstruction{};
  c.info.mode = r->reconstruction.current;
  if (!c.frame) return 0;
  if (c.h_publish[1] != (unsigned int)r->frame_index) return fail(OVR_HIP_EDEVICE, "[hip] the reconstruction of the frame was not published");
  c.info.valid = 1;
  c.info.levels = c.params.levels;
  c.info.sampled_pixels = c.h_publish[0];
  c.info.filled_pixels = (uint64_t)r->fb_pixels - c.info.sampled_pixels;
  if (c.timed) {
    float rm = 0.f;
    HIP_TRY(hipEventElapsedTime(&rm, c.ev[0], c.ev[1]));
    c.info.reconstruct_ms = rm;
  }
  c.accumulated = r->P.accumulate != 0;
  return 0;
}

int finish_frame_one(ovr_hip_renderer* r)
{
  if (!r->async_pending) return 0;
  HIP_TRY(hipStreamSynchronize(r->stream()));
  r->stats.stale_tiles = 0;
  if (int e = resolve_pool(r)) return e;
  if (int e = read_frame_stats(r)) return e;
  if (frame_kind(r->plan) != FrameKind::March) r->stats.tuning = 0; // a projection, isosurface or slice frame feeds neither the tuner nor the automatic pipeline nor the skipping probe
  else {
    const policy::FrameWork w = frame_work(r);
    tune_after_frame(r, w);
    r->auto_pipe.after_frame(w); // automatic shading pipeline of the next frame
    r->skip.after_frame(w);      // did skipping pay?
  }
  if (r->conv.frame)
    if (int e = read_convergence(r)) return e;
  if (int e = read_reconstruction(r)) return e;
  if (r->d_trace) {
    if (const char* path = getenv("OVR_HIP_TRACE_FILE")) {
      std::vector<unsigned long long> h(r->trace_words);
      HIP_TRY(hipMemcpy(h.data(), r->d_trace, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      if (FILE* f = fopen(path, "wb")) { fwrite(h.data(), sizeof(unsigned long long), h.size(), f); fclose(f); }
    }
  }
  r->async_pending = false;
  r->packed_early = false;
  return 0;
}

} // namespace host
} // namespace ovrhip
