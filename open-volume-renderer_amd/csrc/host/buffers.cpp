// buffers.cpp - allocation and release of the buffers a renderer sizes by its framebuffer, by a frame's work or by a mode: framebuffer sets,
// convergence estimate, reconstruction, request pool, sparse-sampling lists.
#include "state.hpp"

#include <cstdlib>

namespace ovrhip {
namespace host {

// the convergence estimate's buffers: gone with the mode, the framebuffer size or the renderer (ensure_convergence brings them back)
int free_convergence(ovr_hip_renderer* r)
{
  if (r->conv.d_accum_half) HIP_TRY(hipFree(r->conv.d_accum_half));
  if (r->conv.d_grad_keep) HIP_TRY(hipFree(r->conv.d_grad_keep));
  if (r->conv.d_error) HIP_TRY(hipFree(r->conv.d_error));
  if (r->conv.d_frames) HIP_TRY(hipFree(r->conv.d_frames));
  if (r->conv.d_words) HIP_TRY(hipFree(r->conv.d_words));
  if (r->conv.d_lists) HIP_TRY(hipFree(r->conv.d_lists));
  r->conv.d_accum_half = r->conv.d_grad_keep = r->conv.d_error = nullptr;
  r->conv.d_frames = nullptr; r->conv.d_words = r->conv.d_lists = nullptr;
  r->conv.blocks = r->conv.list_cap = 0;
  r->conv.valid = false;
  r->conv.active = r->conv.retired = 0;
  return 0;
}

int ensure_convergence(ovr_hip_renderer* r, bool lists)
{
  const int W = r->fbsize.current.w, H = r->fbsize.current.h;
  const size_t n = r->fb_pixels, blocks = (size_t)((W + 7) / 8) * (size_t)((H + 7) / 8);
  const bool adaptive = r->convergence.current.mode == OVR_HIP_CONVERGENCE_ADAPTIVE;
  if (!r->conv.d_accum_half) {
    HIP_TRY(hipMalloc((void**)&r->conv.d_accum_half, std::max<size_t>(n, 1) * 4 * sizeof(float)));
    HIP_TRY(hipMemset(r->conv.d_accum_half, 0, std::max<size_t>(n, 1) * 4 * sizeof(float))); // pixels no frame writes (other ranks' tiles) read 0
  }
  if (!r->conv.d_error || r->conv.blocks != blocks) {
    if (r->conv.d_error) HIP_TRY(hipFree(r->conv.d_error));
    if (r->conv.d_frames) HIP_TRY(hipFree(r->conv.d_frames));
    r->conv.d_error = nullptr; r->conv.d_frames = nullptr;
    HIP_TRY(hipMalloc((void**)&r->conv.d_error, std::max<size_t>(blocks, 1) * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&r->conv.d_frames, std::max<size_t>(blocks, 1) * sizeof(int)));
    r->conv.blocks = blocks;
  }
  if (!r->conv.d_words) {
    HIP_TRY(hipMalloc((void**)&r->conv.d_words, 4 * sizeof(unsigned int)));
    HIP_TRY(hipMemset(r->conv.d_words, 0, 4 * sizeof(unsigned int)));
  }
  if (!r->conv.h_publish) {
    HIP_TRY(hipHostMalloc((void**)&r->conv.h_publish, 4 * sizeof(unsigned int), hipHostMallocDefault));
    std::memset(r->conv.h_publish, 0, 4 * sizeof(unsigned int));
  }
  if (adaptive && lists) { // (sized by the launch list: asked for once the frame has built it)
    if (!r->conv.d_grad_keep) HIP_TRY(hipMalloc((void**)&r->conv.d_grad_keep, std::max<size_t>(n, 1) * 3 * sizeof(float)));
    if (!r->conv.d_lists || r->conv.list_cap < r->sched.n) {
      if (r->conv.d_lists) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(r->conv.d_lists)); }
      r->conv.d_lists = nullptr;
      const size_t cap = std::max<size_t>(r->sched.n, 1);
      HIP_TRY(hipMalloc((void**)&r->conv.d_lists, (2 * cap + (cap + 1023) / 1024) * sizeof(unsigned int)));
      r->conv.list_cap = cap;
    }
  }
  return 0;
}

// the reconstruction's buffers: gone with the mode, the framebuffer size or the renderer (ensure_reconstruction brings them back, zeroed)
int free_reconstruction(ovr_hip_renderer* r)
{
  if (r->recon.d_count) HIP_TRY(hipFree(r->recon.d_count));
  if (r->recon.d_grad) HIP_TRY(hipFree(r->recon.d_grad));
  if (r->recon.d_pyramid) HIP_TRY(hipFree(r->recon.d_pyramid));
  if (r->recon.d_words) HIP_TRY(hipFree(r->recon.d_words));
  r->recon.d_count = r->recon.d_grad = nullptr;
  r->recon.d_pyramid = nullptr;
  r->recon.d_words = nullptr;
  r->recon.frame = r->recon.accumulated = false;
  r->recon.info = ovr_hip_reconstruction{};
  r->recon.info.mode = r->reconstruction.current;
  return 0;
}

// everything the shadow cache holds on the device (the counters of ovr_hip_get_shadow_cache stay)
void free_shadow_cache(ovr_hip_renderer* r)
{
  ShadowCacheState& c = r->shadow_cache;
  if (c.d_built) (void)hipFree(c.d_built);
  if (c.d_supplied) (void)hipFree(c.d_supplied);
  if (c.d_iterations) (void)hipFree(c.d_iterations);
  for (int i = 0; i < 2; ++i) if (c.ev[i]) (void)hipEventDestroy(c.ev[i]);
  c.d_built = c.d_supplied = nullptr;
  c.d_iterations = nullptr;
  c.ev[0] = c.ev[1] = nullptr;
  c.built_cap = 0;
  c.built_valid = false;
  for (int k = 0; k < 3; ++k) c.built_dims[k] = c.supplied_dims[k] = 0;
}

int ensure_reconstruction(ovr_hip_renderer* r)
{
  const size_t n = std::max<size_t>(r->fb_pixels, 1);
  if (!r->recon.d_count) {
    HIP_TRY(hipMalloc((void**)&r->recon.d_count, n * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&r->recon.d_grad, n * 3 * sizeof(float)));
    HIP_TRY(hipMemset(r->recon.d_count, 0, n * sizeof(float)));
    HIP_TRY(hipMemset(r->recon.d_grad, 0, n * 3 * sizeof(float)));
    ReconParams c{};
    c.width = r->fbsize.current.w; c.height = r->fbsize.current.h;
    const size_t texels = recon_plan(c);
    HIP_TRY(hipMalloc((void**)&r->recon.d_pyramid, std::max<size_t>(texels, 1) * 2 * sizeof(float4)));
    HIP_TRY(hipMalloc((void**)&r->recon.d_words, kReconWords * sizeof(unsigned int)));
    HIP_TRY(hipMemset(r->recon.d_words, 0, kReconWords * sizeof(unsigned int)));
  }
  if (!r->recon.h_publish) {
    HIP_TRY(hipHostMalloc((void**)&r->recon.h_publish, 2 * sizeof(unsigned int), hipHostMallocDefault));
    std::memset(r->recon.h_publish, 0, 2 * sizeof(unsigned int));
  }
  for (int i = 0; i < 2; ++i)
    if (!r->recon.ev[i]) HIP_TRY(hipEventCreate(&r->recon.ev[i]));
  return 0;
}

int free_framebuffers(ovr_hip_renderer* r)
{
  for (int i = 0; i < 2; ++i) {
    if (r->d_rgba[i]) HIP_TRY(hipFree(r->d_rgba[i]));
    if (r->d_grad[i]) HIP_TRY(hipFree(r->d_grad[i]));
    if (r->h_rgba[i]) HIP_TRY(hipHostFree(r->h_rgba[i]));
    if (r->h_grad[i]) HIP_TRY(hipHostFree(r->h_grad[i]));
    r->d_rgba[i] = r->d_grad[i] = r->h_rgba[i] = r->h_grad[i] = nullptr;
  }
  if (r->d_accum) HIP_TRY(hipFree(r->d_accum));
  r->d_accum = nullptr;
  if (int e = free_convergence(r)) return e;
  if (int e = free_reconstruction(r)) return e;
  if (r->d_rgba8) HIP_TRY(hipFree(r->d_rgba8));
  if (r->h_rgba8) HIP_TRY(hipHostFree(r->h_rgba8));
  r->d_rgba8 = nullptr; r->h_rgba8 = nullptr;
  if (r->d_rgba16f) HIP_TRY(hipFree(r->d_rgba16f));
  if (r->h_rgba16f) HIP_TRY(hipHostFree(r->h_rgba16f));
  r->d_rgba16f = nullptr; r->h_rgba16f = nullptr;
  if (r->d_spp_rgba) HIP_TRY(hipFree(r->d_spp_rgba));
  if (r->d_spp_grad) HIP_TRY(hipFree(r->d_spp_grad));
  r->d_spp_rgba = r->d_spp_grad = nullptr;
  if (r->d_block_counters) HIP_TRY(hipFree(r->d_block_counters));
  r->d_block_counters = nullptr;
  if (r->sched.d_src) HIP_TRY(hipFree(r->sched.d_src));
  if (r->sched.d_sorted) HIP_TRY(hipFree(r->sched.d_sorted));
  r->sched.d_src = r->sched.d_sorted = nullptr;
  r->sched.n = 0;
  r->sched.list_dirty = r->sched.dirty = true;
  r->sched.clear_gen++;
  if (r->pool.tile_first) HIP_TRY(hipFree(r->pool.tile_first));
  if (r->pool.tile_count) HIP_TRY(hipFree(r->pool.tile_count));
  if (r->pool.pix_state) HIP_TRY(hipFree(r->pool.pix_state));
  r->pool.tile_first = nullptr; r->pool.tile_count = nullptr; r->pool.pix_state = nullptr;
  if (r->d_sparse_xy) HIP_TRY(hipFree(r->d_sparse_xy));
  if (r->d_block_counts) HIP_TRY(hipFree(r->d_block_counts));
  r->d_sparse_xy = nullptr;
  r->d_block_counts = nullptr;
  r->sparse_pixels = 0;
  r->fb_pixels = 0;
  return 0;
}

int resize_framebuffers(ovr_hip_renderer* r, int w, int h)
{
  HIP_TRY(hipDeviceSynchronize()); // device_impl.cpp:117 stops all async rendering first
  if (int e = free_framebuffers(r)) return e;
  const size_t n = (size_t)w * (size_t)h;
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(hipMalloc((void**)&r->d_rgba[i], n * 4 * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&r->d_grad[i], n * 3 * sizeof(float)));
    HIP_TRY(hipMemset(r->d_rgba[i], 0, n * 4 * sizeof(float)));
    HIP_TRY(hipMemset(r->d_grad[i], 0, n * 3 * sizeof(float)));
  }
  HIP_TRY(hipMalloc((void**)&r->d_accum, n * 4 * sizeof(float)));
  HIP_TRY(hipMemset(r->d_accum, 0, n * 4 * sizeof(float)));
  // workgroups of the march: 8x8 pixels (4 waves x 16 rays) in dense mode, 64 list entries in sparse mode
  const size_t nblk = std::max<size_t>((size_t)((w + 7) / 8) * (size_t)((h + 7) / 8), (n + 63) / 64) + 1;
  HIP_TRY(hipMalloc((void**)&r->d_block_counters, nblk * kBlockCounters * sizeof(unsigned int)));
  HIP_TRY(hipMalloc((void**)&r->pool.tile_first, nblk * 4 * sizeof(int)));
  HIP_TRY(hipMalloc((void**)&r->pool.tile_count, nblk * 4 * sizeof(unsigned int)));
  HIP_TRY(hipMalloc((void**)&r->pool.pix_state, std::max<size_t>(n, 1) * sizeof(float4)));
  r->pool_tiles = nblk * 4;
  if (r->d_trace) { HIP_TRY(hipFree(r->d_trace)); r->d_trace = nullptr; }
  if (const char* tr = getenv("OVR_HIP_TRACE")) {
    if (tr[0] == '1') {
      r->trace_words = nblk * 4 * 4;
      HIP_TRY(hipMalloc((void**)&r->d_trace, r->trace_words * sizeof(unsigned long long)));
    }
  }
  r->fb_pixels = n;
  for (int i = 0; i < 2; ++i)
    for (int k = 0; k < 4; ++k) r->d_rect[i][k] = r->h_rgba_rect[i][k] = r->h_grad_rect[i][k] = 0;
  return 0;
}

int ensure_pool(ovr_hip_renderer* r, size_t chunks)
{
  // kPoolSubs sub-pools of equal size, each a multiple of 16 chunks (the largest reservation)
  const size_t sub = ((chunks + kPoolSubs - 1) / kPoolSubs + 15) / 16 * 16;
  chunks = sub * kPoolSubs;
  if (r->pool.reqs && r->pool.capacity >= chunks) return 0;
  HIP_TRY(hipDeviceSynchronize());
  if (r->pool.reqs) HIP_TRY(hipFree(r->pool.reqs));
  if (r->pool.chunk_next) HIP_TRY(hipFree(r->pool.chunk_next));
  if (r->pool.chunk_n) HIP_TRY(hipFree(r->pool.chunk_n));
  if (r->pool.order) HIP_TRY(hipFree(r->pool.order));
  if (r->pool.order_key) HIP_TRY(hipFree(r->pool.order_key));
  r->pool.reqs = nullptr; r->pool.chunk_next = nullptr; r->pool.chunk_n = nullptr; r->pool.order = nullptr; r->pool.order_key = nullptr; r->pool.capacity = 0; r->pool.sub_capacity = 0;
  HIP_TRY(hipMalloc((void**)&r->pool.reqs, chunks * 64 * 32));
  HIP_TRY(hipMalloc((void**)&r->pool.chunk_next, chunks * sizeof(int)));
  HIP_TRY(hipMalloc((void**)&r->pool.chunk_n, chunks * sizeof(unsigned int)));
  HIP_TRY(hipMalloc((void**)&r->pool.order, (chunks / 4 + 1) * sizeof(unsigned int))); // one entry per run of 4 chunks (shade order by light beams)
  HIP_TRY(hipMalloc((void**)&r->pool.order_key, (chunks / 4 + 1) * sizeof(unsigned int)));
  HIP_TRY(hipMemset(r->pool.order_key, 0xff, (chunks / 4 + 1) * sizeof(unsigned int)));
  if (!r->pool.order_ws) {
    HIP_TRY(hipMalloc((void**)&r->pool.order_ws, (size_t)kOrderWsWords * sizeof(unsigned int)));
    HIP_TRY(hipMemset(r->pool.order_ws, 0, (size_t)kOrderWsWords * sizeof(unsigned int))); // the shade kernel leaves the histogram zeroed for the next generation
  }
  r->pool.capacity = (unsigned int)chunks;
  r->pool.sub_capacity = (unsigned int)sub;
  return 0;
}

int ensure_sparse_buffers(ovr_hip_renderer* r)
{
  const size_t n = r->fb_pixels;
  if (r->sparse_pixels == n && r->d_sparse_xy) return 0;
  if (r->d_sparse_xy) HIP_TRY(hipFree(r->d_sparse_xy));
  if (r->d_block_counts) HIP_TRY(hipFree(r->d_block_counts));
  HIP_TRY(hipMalloc((void**)&r->d_sparse_xy, n * 2 * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&r->d_block_counts, sparse_mask_workspace_elems(r->fbsize.current.w, r->fbsize.current.h) * sizeof(unsigned int)));
  r->sparse_pixels = n;
  return 0;
}

} // namespace host
} // namespace ovrhip
