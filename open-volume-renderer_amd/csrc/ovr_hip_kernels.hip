// ovr_hip_kernels.hip - gfx950 (MI355X, CDNA4) kernels of the OVR ray-marching path.
//
// Hand-written for wave64 / 256 CUs / 160 KiB LDS; no CUDA dual path.  Semantics follow the reference's in-tree ray
// marcher (citations relative to the reference tree):
//   raygen + accumulation ........ ovr/devices/optix7/shaders_raymarching.cu:323-413
//   box test ..................... ovr/devices/optix7/shaders_common.h:156-184,379-392
//   marching loop ................ shaders_raymarching.cu:87-171   shadow march :44-85,205-229
//   volume tap / gradient / TF ... shaders_common.h:186-215,311-319,356-367
//   TEA RNG ...................... ovr/common/random/random.h:146-188
//   sparse-sampling mask ......... ovr/common/generate_mask.cu:55-120, ovr/common/random/blue_noise.h:81-102
//
// Kernel shape: FOUR LANES PER RAY - the 4 lanes of a quad are 4 consecutive steps of one ray - so a wave64 marches 16 rays
// (a 4x4-pixel tile) and a workgroup of four waves an 8x8-pixel block; workgroups run longest rays first (launch_schedule).
// Shaded samples become 32-byte requests that a second, persistent kernel shades from a global pool and a third kernel
// composites in ray order (pooled pipeline), or that the tile's own wave shades (in-place pipeline).  The transfer
// function (colour float4 table + alpha table, 20 KiB at the shipped resolution of 1024), the per-axis brick-offset tables,
#include "ovr_hip_device.h"
#include "ovr_hip_isosurface_ao.h"
#include "ovr_hip_slices.h"
#include "ovr_hip_slice_context.h"
#include "ovr_hip_preintegration.h"
#include "ovr_hip_gradient_opacity.h"
#include "ovr_hip_max_depth.h"
#include "ovr_hip_depth_output.h"
#include "ovr_hip_isosurface_context.h"
#include "ovr_hip_update.h"
#include "host/ray_query.hpp"

namespace ovrhip {
static_assert(kPoolSubs <= 64 && (kPoolSubs & (kPoolSubs - 1)) == 0, "reduce_counters_kernel reduces the sub-pool counters with one wave");
// ------------------------------------------------------------------------------------------------------------------
// pooled pipeline, kernel C: every tile walks its chunks in order, composites and writes its pixels
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void composite_kernel(const RayMarchParams P)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int ix, iy;
  const bool active = assign_pixel_quad(P, lane, wave, ix, iy) && (lane & 3) == 0; // one owner lane per ray, as in the march
  const PoolDesc& Q = P.pool;
  if (Q.ctrl[1] != 0u) return; // pool overflow: the host re-renders this frame with a larger pool, nothing may be written
  const unsigned int tile = blockIdx.x * kWaves + wave;
  const unsigned int pixel_index = (unsigned int)ix + (unsigned int)iy * (unsigned int)P.width;
  float alpha = 0.f;
  unsigned int first = 0;
  int pend = 0;
  if (active) {
    const float4 st = Q.pix_state[pixel_index];
    alpha = st.x; first = __float_as_uint(st.y); pend = __float_as_int(st.z);
  }
  f3 color = mk3(0, 0, 0), gradient = mk3(0, 0, 0);
  // The tile's chunks come in runs of kRun consecutive, kRun-aligned pool slots (the march reserves them that way), so
  // inside a run the next chunk is c + 1 and only the run-to-run link (chunk_next of the run's last slot) is chased - it
  // is fetched when the run is entered, a whole run ahead of its use.  The next chunk's requests are loaded before the
  // current ones are applied, so the walk no longer pays two dependent memory latencies per chunk.
  const unsigned int total = Q.tile_count[tile];
  auto load_chunk = [&](int c, unsigned int n) {
    ShadeReq r;
    r.px = r.py = r.pz = r.s = r.v = r.tr = r.a = 0.f; r.next = 0;
    if ((unsigned int)lane < n) r = Q.reqs[(size_t)c * 64 + lane];
    return r;
  };
  int c = total > 0u ? Q.tile_first[tile] : 0;
  int link = total > 0u ? Q.chunk_next[c | (kRun - 1)] : 0;
  ShadeReq r = load_chunk(c, min(total, 64u));
  for (unsigned int base = 0; base < total; base += 64u) {
    const unsigned int n = min(total - base, 64u);
    const bool more = base + 64u < total;
    const bool run_end = (c & (kRun - 1)) == kRun - 1;
    const int c_next = run_end ? link : c + 1;
    ShadeReq r_next = r;
    if (more) {
      r_next = load_chunk(c_next, min(total - base - 64u, 64u));
      if (run_end) link = Q.chunk_next[c_next | (kRun - 1)];
    }
    apply_batch(r, base, n, lane, pend, first, color, gradient);
    r = r_next;
    c = c_next;
  }
  if (active) {
    f3 o_c = mk3(0, 0, 0), o_g = mk3(0, 0, 0);
    if (alpha > 0.f) {
      o_c = mk3(color.x / alpha, color.y / alpha, color.z / alpha);
      o_g = mk3(gradient.x / alpha, gradient.y / alpha, gradient.z / alpha);
    }
    float o_a = alpha;
    if (P.spp > 1) {
      // one launch per sample-per-pixel generation: sum the generations in order (shaders_raymarching.cu:351-376)
      float4* sr = reinterpret_cast<float4*>(P.spp_sum_rgba) + pixel_index;
      float* sg = P.spp_sum_grad + 3ull * pixel_index;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      f3 accg = mk3(0, 0, 0);
      if (P.spp_index > 0) { acc = *sr; accg = mk3(sg[0], sg[1], sg[2]); }
      acc.x += o_c.x; acc.y += o_c.y; acc.z += o_c.z; acc.w += alpha;
      accg.x += o_g.x; accg.y += o_g.y; accg.z += o_g.z;
      if (P.spp_index + 1 < P.spp) {
        *sr = acc; sg[0] = accg.x; sg[1] = accg.y; sg[2] = accg.z;
        return;
      }
      if (Q.ctrl[32 * (kPoolSubs + 1)] > Q.sub_capacity) return; // an earlier generation overflowed the pool: the whole frame is re-rendered
      const float rspp = 1.f / (float)P.spp;
      o_a = acc.w * rspp;
      o_c = mk3(acc.x * rspp, acc.y * rspp, acc.z * rspp);
      o_g = mk3(accg.x * rspp, accg.y * rspp, accg.z * rspp);
    }
    // spp == 1: (x + 0) * (1 / 1) is exact, so this equals the in-place kernel's o_c * rspp bit for bit
    write_pixel(P, pixel_index, o_c, o_a, o_g);
  }
}

// sums the per-workgroup partials into counters[0..4]: each workgroup reduces a slice and adds its 5 sums with one
// atomic each (integer sums: the result does not depend on the order); counters are zeroed by a memset node before
__global__ __launch_bounds__(256) void reduce_counters_kernel(const unsigned int* __restrict__ partials, int n_blocks, const unsigned int* __restrict__ shade_partials,
                                                             int n_shade_blocks, unsigned long long* counters, unsigned int* pool_ctrl,
                                                             unsigned long long* publish, unsigned int* done, unsigned int* conv_asked)
{
  if (pool_ctrl && blockIdx.x == 0 && threadIdx.x < 64) { // most chunks any sub-pool was asked for in any generation (kPoolSubs == 64: one wave)
    unsigned int v = threadIdx.x < (unsigned int)kPoolSubs ? pool_ctrl[32u * (threadIdx.x + 1u)] : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned int)__shfl_xor((int)v, off));
    if (threadIdx.x == 0) atomicMax(&pool_ctrl[32 * (kPoolSubs + 1)], v);
  }
  __shared__ unsigned long long red[4][kNC];
  unsigned long long acc[kNC] = {};
  const int stride = gridDim.x * 256;
  for (int b = blockIdx.x * 256 + threadIdx.x; b < n_blocks; b += stride) {
#pragma unroll
    for (int c = 0; c < kNC; ++c) acc[c] += partials[(size_t)b * kNC + c];
  }
  if (shade_partials)
    for (int b = blockIdx.x * 256 + threadIdx.x; b < n_shade_blocks; b += stride) {
      acc[3] += shade_partials[2 * b];
      acc[6] += shade_partials[2 * b + 1];
    }
#pragma unroll
  for (int c = 0; c < kNC; ++c) {
    for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_down(acc[c], off);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kNC; ++c) red[wave][c] = acc[c];
  }
  __syncthreads();
  if (threadIdx.x < kNC) atomicAdd(&counters[threadIdx.x], red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
  if (!publish) return; // the old protocol, or an earlier generation of a frame with several samples per pixel: the sums go on accumulating
  // The workgroup that finishes last hands the frame's totals and the pool's control words to the host (pinned memory: visible when the
  // stream has been synchronised) and leaves both zeroed for the next frame: no memset in front of a frame, no copy behind it.
  __shared__ unsigned int ticket;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) ticket = atomicAdd(done, 1u);
  __syncthreads();
  if (ticket != gridDim.x - 1u) return;
  __threadfence();
  if (threadIdx.x < 8) {
    publish[threadIdx.x] = threadIdx.x < kNC ? __hip_atomic_load(&counters[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    counters[threadIdx.x] = 0ull;
  }
  unsigned int* pub_ctrl = reinterpret_cast<unsigned int*>(publish + 8);
  if (pool_ctrl)
    for (int i = threadIdx.x; i < kPoolCtrlWords; i += 256) {
      const unsigned int w = __hip_atomic_load(&pool_ctrl[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pub_ctrl[i] = w;
      pool_ctrl[i] = 0u;
      if (conv_asked && i == 32 * (kPoolSubs + 1)) *conv_asked = w; // for the convergence kernels behind this frame (RayMarchParams::conv_asked)
    }
  else if (conv_asked && threadIdx.x == 0) *conv_asked = 0u;
  if (threadIdx.x == 0) *done = 0u;
}
// ------------------------------------------------------------------------------------------------------------------
// launch order of the march workgroups: longest rays first
// A wave needs as long as its longest ray (~1700 dependent steps through the volume's diagonal), however empty the machine
// is; in launch-index order those waves sit in the middle of the grid and the kernel ends with a tail of a few hundred
// microseconds at a fraction of the occupancy (per-wave trace: the last 15 % of the march's time ran < 1/3 of the waves;
// on an image shard, where the kernel is 4-8 x shorter, the tail was half of it).  Sorting the owned 8x8 blocks by the
// length of their rays' box intersection (counting sort, 64 classes, descending) starts the long ones first and lets the
// short ones fill the gaps.  One workgroup; runs when the camera, the framebuffer size, the volume's box or the shard changes.
// ------------------------------------------------------------------------------------------------------------------
constexpr int kSchedClasses = 64;
// length of probe ray k of block e inside the box (k = 0: the block's centre, 1 ... 4: its corners), -1 = it misses
template <bool CLIP, bool ORTHO>
__device__ __forceinline__ float schedule_probe(const RayMarchParams& P, const MarchConsts& mc, unsigned int e, int k)
{
  const int bx = (int)(e & 0xffffu) * 8, by = (int)(e >> 16) * 8;
  const int ix = min(bx + (k == 0 ? 4 : (k & 1) ? 0 : 7), P.width - 1), iy = min(by + (k == 0 ? 4 : (k & 2) ? 0 : 7), P.height - 1);
  const float ux = ((float)ix + .5f) / (float)P.width - 0.5f, uy = ((float)iy + .5f) / (float)P.height - 0.5f;
  f3 o, d;
  pixel_ray<ORTHO>(P, ux, uy, o, d);
  const f3 oo = to_object(mc, o);
  float a = 0.f, b = FLT_MAX;
  if (primary_box_test<CLIP, ORTHO>(P, a, b, oo, mk3(d.x * mc.inv_scale.x, d.y * mc.inv_scale.y, d.z * mc.inv_scale.z))) return b - a;
  return -1.f;
}
// the block's class from the longest of its five probe rays: 0 = none meets the volume (last), 1 ... kSchedClasses - 1 by length
__device__ __forceinline__ unsigned int schedule_class_of(const RayMarchParams& P, float longest)
{
  if (!(longest >= 0.f)) return 0u;
  const float rel = longest / (P.long_ray_steps * P.step); // 1 = the volume's diagonal
  return (unsigned int)min(kSchedClasses - 1, 1 + (int)(rel * (float)(kSchedClasses - 2)));
}

// Three launches (a single workgroup needed 0.35 ms for the 32 400 blocks of a 1080p frame - on every camera change, i.e. on every frame of
// an interactive session), nothing in front of them and no copy behind (`tools/camera_move_breakdown.py`):
//   schedule_hist_kernel     ceil(n / 1024) workgroups: one histogram row per workgroup, hist[wg][class], + the active pixels of its class-0 blocks
//   schedule_scatter_kernel  workgroup wg's blocks of class c start at (all blocks of longer classes) + (class-c blocks of the
//                            workgroups before wg); inside the workgroup they keep their list order (stable: the host lists the
//                            blocks supertile by supertile, 4x4 blocks = 32x32 pixels, so blocks that run at the same time are
//                            compact squares of the image and share their bricks in L2 / Infinity Cache).  Workgroup 0 writes `info`
//                            (pinned host memory): how many blocks need a workgroup, the pixels of the others
// (One kernel in which every workgroup counts the whole list itself: 38 us instead of 5 + 10 - the per-wave loop over distinct classes is long
// inside the silhouette, where 64 consecutive entries hold ~20 length classes.)
// (Mapping the 16 blocks of a supertile to ONE XCD - workgroup s runs on XCD s % 8 - was measured slower: C3 march 1.63 vs 1.57 ms.)
//   schedule_classify_kernel one WAVE per block: its length class (five probe rays, one per lane) and - `exact` - whether ANY of its 64 pixel rays meets the box
//                            (pixel_ray_hits_box: the march's own test); cls[i] = class | active pixels << 8, class 0 <=> (exact) no ray hits
//                            CLIP: both against the committed clip box, as the clipped march tests it (the frustum culling of exact == 2 keeps the
//                            volume's own box: a superset)
//                            ORTHO: the orthographic camera's rays (pixel_ray, primary_box_test), on the clipped test; exact == 2 culls by rectangles - the
//                            planes of the frustum cull meet in the eye, which parallel rays do not have: see below
template <bool CLIP, bool ORTHO = false>
__global__ __launch_bounds__(256) void schedule_classify_kernel(const RayMarchParams P, const unsigned int* __restrict__ src, unsigned int n, int exact,
                                                               unsigned int* __restrict__ cls)
{
  VolConsts vc;
  MarchConsts mc;
  setup_consts(P, vc, mc);
  const unsigned int i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= n) return; // wave-uniform
  const int lane = threadIdx.x & 63;
  const unsigned int e = src[i];
  const int ix = (int)(e & 0xffffu) * 8 + (lane & 7), iy = (int)(e >> 16) * 8 + (lane >> 3);
  bool active = ix < P.width && iy < P.height;
  if (P.world > 1 && active) active = ((ix / P.tile_w + iy / P.tile_h) % P.world) == P.rank; // assign_pixel_quad's ownership test
  const bool hit = exact == 1 && active && pixel_ray_hits_box<CLIP, ORTHO>(P, mc, ix, iy);
  const unsigned long long any = __ballot(hit), act = __ballot(active);
  // exact == 2 (several samples per pixel, or jittered ones: a pixel's rays are only known to lie within half a pixel of its centre): the block
  // is surely empty if the cone of ALL rays through the block widened by 1.5 pixels lies beyond one of its own four side planes from the whole
  // box (frustum culling: 4 planes x 8 box corners, one pair per lane, object space), and no ray in it can have a direction component near 0
  // (the reference's box test ignores the slab of such a component, shaders_common.h:162-172: a ray could then "hit" from outside the silhouette)
  bool culled = false;
  if (exact == 2 && ORTHO) {
    // parallel rays: a ray's origin is cam_pos + ux hor + uy ver, and it can only meet the box if (ux, uy) lies inside the rectangle that bounds the box's
    // eight corners projected along cam_dir onto (hor, ver).  The block's rays have (ux, uy) inside its pixel rectangle widened by 1.5 pixels (any jitter);
    // the block is surely empty if the two rectangles are apart by more than a margin far above the rounding of the projections.  The volume's own box, like
    // the frustum cull: a superset of a clip box.  (Under this camera a ray outside an ignored slab misses, so no sign condition is needed.)
    const float x0 = ((float)((int)(e & 0xffffu) * 8) - 1.5f) / (float)P.width - 0.5f, x1 = ((float)((int)(e & 0xffffu) * 8 + 8) + 1.5f) / (float)P.width - 0.5f;
    const float y0 = ((float)((int)(e >> 16) * 8) - 1.5f) / (float)P.height - 0.5f, y1 = ((float)((int)(e >> 16) * 8 + 8) + 1.5f) / (float)P.height - 0.5f;
    const f3 cp = ld3(P.cam_pos), ch = ld3(P.cam_hor), cv = ld3(P.cam_ver);
    const int cn = lane & 7; // one corner per lane, eight lanes hold the box
    const f3 w = mk3(((float)(cn & 1) - mc.wto_p.x) / mc.inv_scale.x - cp.x, ((float)((cn >> 1) & 1) - mc.wto_p.y) / mc.inv_scale.y - cp.y,
                     ((float)(cn >> 2) - mc.wto_p.z) / mc.inv_scale.z - cp.z);
    const float su = dot3(w, ch) / dot3(ch, ch), sv = dot3(w, cv) / dot3(cv, cv);
    float ulo = su, uhi = su, vlo = sv, vhi = sv;
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
      ulo = fminf(ulo, __shfl_xor(ulo, off)); uhi = fmaxf(uhi, __shfl_xor(uhi, off));
      vlo = fminf(vlo, __shfl_xor(vlo, off)); vhi = fmaxf(vhi, __shfl_xor(vhi, off));
    }
    const float margin = 1e-4f * (1.f + fmaxf(fmaxf(fabsf(ulo), fabsf(uhi)), fmaxf(fabsf(vlo), fabsf(vhi))));
    culled = x1 < ulo - margin || x0 > uhi + margin || y1 < vlo - margin || y0 > vhi + margin; // (a NaN compares false: not culled)
  }
  if (exact == 2 && !ORTHO) {
    const float x0 = ((float)((int)(e & 0xffffu) * 8) - 1.5f) / (float)P.width - 0.5f, x1 = ((float)((int)(e & 0xffffu) * 8 + 8) + 1.5f) / (float)P.width - 0.5f;
    const float y0 = ((float)((int)(e >> 16) * 8) - 1.5f) / (float)P.height - 0.5f, y1 = ((float)((int)(e >> 16) * 8 + 8) + 1.5f) / (float)P.height - 0.5f;
    const f3 cd = ld3(P.cam_dir), ch = ld3(P.cam_hor), cv = ld3(P.cam_ver);
    auto ray = [&](int k) { // corner k of the widened block, counter-clockwise; object-space direction (not normalised)
      const float ux = (k == 1 || k == 2) ? x1 : x0, uy = (k >= 2) ? y1 : y0;
      return mk3((cd.x + ux * ch.x + uy * cv.x) * mc.inv_scale.x, (cd.y + ux * ch.y + uy * cv.y) * mc.inv_scale.y, (cd.z + ux * ch.z + uy * cv.z) * mc.inv_scale.z);
    };
    const f3 oo = to_object(mc, ld3(P.cam_pos));
    const int pl = (lane >> 3) & 3, cn = lane & 7;
    const f3 a = ray(pl), b = ray((pl + 1) & 3), in = ray((pl + 2) & 3);
    const f3 nrm = mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
    const float side = dot3(nrm, in);                                          // the sign of the cone's inside
    const f3 v = mk3((float)(cn & 1) - oo.x, (float)((cn >> 1) & 1) - oo.y, (float)(cn >> 2) - oo.z);
    const float d = dot3(nrm, v) * (side >= 0.f ? 1.f : -1.f);
    const float scale = sqrtf(dot3(nrm, nrm) * dot3(v, v));
    const bool outside = lane < 32 && fabsf(side) > 0.f && d < -1e-4f * scale;   // this corner lies beyond this plane, with a margin far above the rounding of the products
    const unsigned int bits = (unsigned int)__ballot(outside);
    bool beyond = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) beyond = beyond || ((bits >> (8 * k)) & 0xffu) == 0xffu;
    // direction components over the widened block: linear in (ux, uy), so the extremes are at the corners
    bool sign_safe = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float c00 = k == 0 ? ray(0).x : k == 1 ? ray(0).y : ray(0).z, c10 = k == 0 ? ray(1).x : k == 1 ? ray(1).y : ray(1).z;
      const float c11 = k == 0 ? ray(2).x : k == 1 ? ray(2).y : ray(2).z, c01 = k == 0 ? ray(3).x : k == 1 ? ray(3).y : ray(3).z;
      const float lo = fminf(fminf(c00, c10), fminf(c11, c01)), hi = fmaxf(fmaxf(c00, c10), fmaxf(c11, c01));
      const float len = sqrtf(dot3(ray(0), ray(0)));
      sign_safe = sign_safe && (lo > 1e-6f * len || hi < -1e-6f * len);
    }
    culled = beyond && sign_safe;
  }
  float longest = lane < 5 ? schedule_probe<CLIP, ORTHO>(P, mc, e, lane) : -1.f; // (until round 4 lane 0 traced all five: 58 us per camera change at 1080p)
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) longest = fmaxf(longest, __shfl_xor(longest, off));
  if (lane == 0) {
    unsigned int c = schedule_class_of(P, longest);
    if (exact == 1) c = any != 0ull ? max(c, 1u) : 0u;
    if (exact == 2) c = culled ? 0u : max(c, 1u);
    cls[i] = c | ((unsigned int)__popcll(act) << 8);
  }
}

constexpr int kSchedRow = kSchedClasses + 1; // a workgroup's histogram row: its class counts, then the active pixels of its class-0 blocks
__global__ __launch_bounds__(1024) void schedule_hist_kernel(const unsigned int* __restrict__ cls, unsigned int n, unsigned int* __restrict__ hist)
{
  __shared__ unsigned int count[kSchedRow];
  if (threadIdx.x < kSchedRow) count[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned int i = blockIdx.x * 1024u + threadIdx.x;
  if (i < n) {
    const unsigned int c = cls[i];
    atomicAdd(&count[c & 0xffu], 1u);
    if ((c & 0xffu) == 0u) atomicAdd(&count[kSchedClasses], c >> 8);
  }
  __syncthreads();
  if (threadIdx.x < kSchedRow) hist[blockIdx.x * kSchedRow + threadIdx.x] = count[threadIdx.x];
}

__global__ __launch_bounds__(1024) void schedule_scatter_kernel(const unsigned int* __restrict__ src, const unsigned int* __restrict__ cls_in, unsigned int n,
                                                                const unsigned int* __restrict__ hist, unsigned int* __restrict__ dst, unsigned int* __restrict__ info)
{
  __shared__ unsigned int base[kSchedRow], total[kSchedRow];
  __shared__ unsigned int wave_count[16][kSchedClasses];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // per class: blocks in the workgroups before this one, and in all of them (last column: the pixels of the class-0 blocks)
  if (threadIdx.x < kSchedRow) {
    unsigned int before = 0u, all = 0u;
    for (unsigned int w = 0; w < gridDim.x; ++w) {
      const unsigned int h = hist[w * kSchedRow + threadIdx.x];
      before += w < blockIdx.x ? h : 0u;
      all += h;
    }
    base[threadIdx.x] = before;
    total[threadIdx.x] = all;
  }
  for (int k = threadIdx.x; k < 16 * kSchedClasses; k += 1024) (&wave_count[0][0])[k] = 0u;
  __syncthreads();
  if (threadIdx.x == 0) { // descending classes: the longest rays first
    unsigned int at = 0u;
    for (int c = kSchedClasses - 1; c >= 0; --c) { const unsigned int t = total[c]; base[c] += at; at += t; }
    // what the host waits for (pinned memory): the blocks that need a workgroup - everything before class 0 - and the active pixels of the others
    if (info && blockIdx.x == 0) { info[0] = n - total[0]; info[1] = total[kSchedClasses]; }
  }
  const unsigned int i = blockIdx.x * 1024u + threadIdx.x;
  const bool valid = i < n;
  const unsigned int e = valid ? src[i] : 0u;
  const unsigned int cls = valid ? (cls_in[i] & 0xffu) : 0u;
  // rank among the lanes of this wave with the same class (lower lanes first), wave totals to LDS
  unsigned int rank = 0u;
  unsigned long long todo = __ballot(valid);
  while (todo != 0ull) {
    const int leader = __builtin_ctzll(todo);
    const unsigned int lc = (unsigned int)__builtin_amdgcn_readlane((int)cls, leader);
    const unsigned long long same = __ballot(valid && cls == lc);
    if (valid && cls == lc) rank = (unsigned int)__popcll(same & ((1ull << lane) - 1ull));
    if (lane == leader) wave_count[wave][lc] = (unsigned int)__popcll(same);
    todo &= ~same;
  }
  __syncthreads();
  // exclusive prefix over the 16 waves, per class
  if (threadIdx.x < kSchedClasses) {
    unsigned int run = base[threadIdx.x];
    for (int w = 0; w < 16; ++w) { const unsigned int t = wave_count[w][threadIdx.x]; wave_count[w][threadIdx.x] = run; run += t; }
  }
  __syncthreads();
  if (valid) dst[wave_count[wave][cls] + rank] = e;
}

size_t schedule_workspace_elems(unsigned int n) { return (size_t)((n + 1023u) / 1024u) * kSchedRow + (size_t)n; } // histogram rows + one class word per block

hipError_t launch_schedule(const RayMarchParams& p, const unsigned int* src, unsigned int n, unsigned int* dst, unsigned int* workspace, int exact, unsigned int* info,
                           hipStream_t stream)
{
  if (n == 0) { // nothing to sort: the caller does not read info
    return hipSuccess;
  }
  const dim3 grid((n + 1023u) / 1024u);
  unsigned int* hist = workspace;
  unsigned int* cls = workspace + (size_t)grid.x * kSchedRow;
  auto classify = p.cam_orthographic ? schedule_classify_kernel<true, true> : p.clip_on ? schedule_classify_kernel<true> : schedule_classify_kernel<false>;
  hipLaunchKernelGGL(classify, dim3((n + 3u) / 4u), dim3(256), 0, stream, p, src, n, exact, cls);
  hipLaunchKernelGGL(schedule_hist_kernel, grid, dim3(1024), 0, stream, cls, n, hist);
  hipLaunchKernelGGL(schedule_scatter_kernel, grid, dim3(1024), 0, stream, src, cls, n, hist, dst, info);
  return hipGetLastError();
}

// the pixels of blocks that are not launched (no ray of theirs meets the box): what the march's miss writes - 0 in every layer
// (shaders_raymarching.cu:237-253 + the accumulation of :389-409: accum += 0, rgba = accum / frame_index = 0)
__global__ __launch_bounds__(256) void clear_blocks_kernel(const RayMarchParams P, const unsigned int* __restrict__ blocks, unsigned int n, int clear_accum)
{
  const unsigned int i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const unsigned int e = blocks[i];
  const int ix = (int)(e & 0xffffu) * 8 + (lane & 7), iy = (int)(e >> 16) * 8 + (lane >> 3);
  bool active = ix < P.width && iy < P.height;
  if (P.world > 1 && active) active = ((ix / P.tile_w + iy / P.tile_h) % P.world) == P.rank;
  if (!active) return;
  const size_t pi = (size_t)ix + (size_t)iy * (size_t)P.width;
  reinterpret_cast<float4*>(P.rgba)[pi] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (P.grad) { float* g = P.grad + 3 * pi; g[0] = 0.f; g[1] = 0.f; g[2] = 0.f; }
  if (clear_accum && P.accum) reinterpret_cast<float4*>(P.accum)[pi] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (clear_accum && P.accum_half) reinterpret_cast<float4*>(P.accum_half)[pi] = make_float4(0.f, 0.f, 0.f, 0.f);
}
hipError_t launch_clear_blocks(const RayMarchParams& p, const unsigned int* blocks, unsigned int n, int clear_accum, hipStream_t stream)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(clear_blocks_kernel, dim3((n + 3u) / 4u), dim3(256), 0, stream, p, blocks, n, clear_accum);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// convergence estimate and adaptive refinement (ConvergenceParams, ovr_hip_kernels.h)
//   convergence_kernel      one wave per block marched by the even frame n: E_b, the block's state, the maxima; a block that retires keeps its gradient pixels
//   convergence_count /     (adaptive) stable compaction of the SORTED launch list by the blocks' states into the active and the retired list: per-workgroup
//   convergence_scatter     counts, then every workgroup adds up the counts in front of it (as schedule_hist / schedule_scatter do); workgroup 0 publishes
//   convergence_publish     (estimate only) one wave publishes
//   resolve_blocks_kernel   every frame after a retirement: a retired block's pixels are A / n_b and the gradient pixels it kept
// Kernel boundaries order everything; all of them return at once behind an attempt that overflowed the request pool (no pixel was written: A and H are
// those of the frame before, the host renders the frame again and these kernels with it).
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool convergence_attempt_void(const ConvergenceParams& C) { return C.words[2] > C.sub_capacity; }

__global__ __launch_bounds__(256) void convergence_kernel(const ConvergenceParams C)
{
  const unsigned int i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= C.n_active) return; // wave-uniform
  if (convergence_attempt_void(C)) return;
  const int lane = threadIdx.x & 63;
  const unsigned int ent = C.active[i];
  const int bx = (int)(ent & 0xffffu), by = (int)(ent >> 16);
  const int ix = bx * 8 + (lane & 7), iy = by * 8 + (lane >> 3);
  bool present = ix < C.width && iy < C.height;
  if (C.world > 1 && present) present = ((ix / C.tile_w + iy / C.tile_h) % C.world) == C.rank; // assign_pixel_quad's ownership test
  const size_t pi = (size_t)(present ? ix : 0) + (size_t)(present ? iy : 0) * (size_t)C.width;
  float e = 0.f;
  if (present) {
    const float4 a = reinterpret_cast<const float4*>(C.accum)[pi], h = reinterpret_cast<const float4*>(C.accum_half)[pi];
    const float fn = (float)C.frame_index, fh = (float)(C.frame_index / 2);
    const float mr = a.x / fn, mg = a.y / fn, mb = a.z / fn, ma = a.w / fn;
    const float hr = h.x / fh, hg = h.y / fh, hb = h.z / fh, ha = h.w / fh;
    const float d = ((fabsf(mr - hr) + fabsf(mg - hg)) + fabsf(mb - hb)) + fabsf(ma - ha);
    const float s = ((mr + mg) + mb) + ma;
    e = s > 0.f ? d / sqrtf(s) : 0.f;
  }
  const int count = (int)__popcll(__ballot(present));
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) e += __shfl_xor(e, off); // the balanced pairwise tree over the lane index: the same value in every lane
  const float E = count > 0 ? e / (float)count : 0.f;
  const bool retire = C.adaptive != 0 && E <= C.threshold;
  if (lane == 0) {
    const size_t b = (size_t)bx + (size_t)by * (size_t)C.blocks_x;
    C.block_error[b] = E;
    C.block_frames[b] = retire ? -C.frame_index : C.frame_index;
    // a maximum only grows: a block that cannot raise what the word already shows (0 for every block of a static scene) sends no atomic - tens of
    // thousands of atomics on one address would serialise in L2; a stale read only costs an atomic that changes nothing
    unsigned int* w = &C.words[retire ? 1 : 0];
    const unsigned int bits = __float_as_uint(E);
    if (bits > __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(w, bits);
  }
  if (retire && present) {
    const float* g = C.grad + 3 * pi;
    float* k = C.grad_keep + 3 * pi;
    k[0] = g[0]; k[1] = g[1]; k[2] = g[2];
  }
}

__device__ __forceinline__ bool convergence_entry_active(const ConvergenceParams& C, unsigned int ent)
{
  return C.block_frames[(size_t)(ent & 0xffffu) + (size_t)(ent >> 16) * (size_t)C.blocks_x] >= 0;
}

__global__ __launch_bounds__(1024) void convergence_count_kernel(const ConvergenceParams C)
{
  if (convergence_attempt_void(C)) return;
  __shared__ unsigned int wave_count[16];
  const unsigned int i = blockIdx.x * 1024u + threadIdx.x;
  const bool keep = i < C.n_work && convergence_entry_active(C, C.sorted[i]);
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = (unsigned int)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int t = 0u;
    for (int w = 0; w < 16; ++w) t += wave_count[w];
    C.counts[blockIdx.x] = t;
  }
}

__device__ __forceinline__ void convergence_publish(const ConvergenceParams& C, unsigned int n_active)
{
  C.publish[0] = max(C.words[0], C.words[1]);
  C.publish[1] = n_active;
  C.publish[2] = C.n_work - n_active;
  C.publish[3] = (unsigned int)C.frame_index;
  C.words[0] = 0u; // the next estimate starts from 0; the retired blocks' maximum stays
}

__global__ __launch_bounds__(1024) void convergence_scatter_kernel(const ConvergenceParams C)
{
  if (convergence_attempt_void(C)) return;
  __shared__ unsigned int wave_base[16];
  __shared__ unsigned int before_s, total_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave == 0) { // the active entries of the workgroups in front of this one, and of all of them
    unsigned int before = 0u, all = 0u;
    for (unsigned int w = (unsigned int)lane; w < gridDim.x; w += 64u) {
      const unsigned int c = C.counts[w];
      before += w < blockIdx.x ? c : 0u;
      all += c;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { before += __shfl_xor(before, off); all += __shfl_xor(all, off); }
    if (lane == 0) { before_s = before; total_s = all; }
  }
  const unsigned int i = blockIdx.x * 1024u + threadIdx.x;
  const bool valid = i < C.n_work;
  const unsigned int ent = valid ? C.sorted[i] : 0u;
  const bool keep = valid && convergence_entry_active(C, ent);
  const unsigned long long m = __ballot(keep);
  const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u)); // kept lanes below this one
  if (lane == 0) wave_base[wave] = (unsigned int)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int run = before_s;
    for (int w = 0; w < 16; ++w) { const unsigned int t = wave_base[w]; wave_base[w] = run; run += t; }
    if (blockIdx.x == 0) convergence_publish(C, total_s);
  }
  __syncthreads();
  if (!valid) return;
  const unsigned int kept_before = wave_base[wave] + rank; // active entries in front of entry i: both lists keep the sorted order
  if (keep) C.active_out[kept_before] = ent;
  else C.retired_out[i - kept_before] = ent;
}

__global__ __launch_bounds__(64) void convergence_publish_kernel(const ConvergenceParams C)
{
  if (convergence_attempt_void(C)) return;
  if (threadIdx.x == 0) convergence_publish(C, C.n_work);
}

hipError_t launch_convergence(const ConvergenceParams& c, hipStream_t stream)
{
  if (c.n_active > 0) hipLaunchKernelGGL(convergence_kernel, dim3((c.n_active + 3u) / 4u), dim3(256), 0, stream, c);
  if (c.adaptive && c.n_work > 0) {
    const dim3 grid((c.n_work + 1023u) / 1024u);
    hipLaunchKernelGGL(convergence_count_kernel, grid, dim3(1024), 0, stream, c);
    hipLaunchKernelGGL(convergence_scatter_kernel, grid, dim3(1024), 0, stream, c);
  }
  else hipLaunchKernelGGL(convergence_publish_kernel, dim3(1), dim3(64), 0, stream, c);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void resolve_blocks_kernel(const RayMarchParams P, const unsigned int* __restrict__ retired, unsigned int n, const int* __restrict__ block_frames,
                                                            const float* __restrict__ grad_keep, int blocks_x)
{
  const unsigned int i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const unsigned int e = retired[i];
  const int ix = (int)(e & 0xffffu) * 8 + (lane & 7), iy = (int)(e >> 16) * 8 + (lane >> 3);
  bool active = ix < P.width && iy < P.height;
  if (P.world > 1 && active) active = ((ix / P.tile_w + iy / P.tile_h) % P.world) == P.rank;
  if (!active) return;
  const float fn = (float)(-block_frames[(size_t)(e & 0xffffu) + (size_t)(e >> 16) * (size_t)blocks_x]); // n_b: the frame the block retired after
  const size_t pi = (size_t)ix + (size_t)iy * (size_t)P.width;
  const float4 a = reinterpret_cast<const float4*>(P.accum)[pi];
  reinterpret_cast<float4*>(P.rgba)[pi] = make_float4(a.x / fn, a.y / fn, a.z / fn, a.w / fn); // write_pixel's expression
  if (P.grad) {
    const float* k = grad_keep + 3 * pi;
    float* g = P.grad + 3 * pi;
    g[0] = k[0]; g[1] = k[1]; g[2] = k[2];
  }
}
hipError_t launch_resolve_blocks(const RayMarchParams& p, const unsigned int* retired, unsigned int n, const int* block_frames, const float* grad_keep, int blocks_x,
                                 hipStream_t stream)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(resolve_blocks_kernel, dim3((n + 3u) / 4u), dim3(256), 0, stream, p, retired, n, block_frames, grad_keep, blocks_x);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// Pull-push reconstruction of sparse-sampled frames (ReconParams, ovr_hip_kernels.h).  The arithmetic is
// open-volume-renderer_amd/reconstruction.py's, operation for operation: every sum is pairwise, x first - what two lane exchanges compute -, every
// invalid child contributes a SELECTED +0, every product and sum of the push is rounded on its own (-ffp-contract=off).
// An 8x8 block of a level is one wave in the lane order of the convergence kernel (lane = 8 * (y & 7) + (x & 7)): three levels come out of the
// exchanges xor 1 / xor 8, xor 2 / xor 16, xor 4 / xor 32 without LDS.  From the first level of at most 64 x 64 texels on, one workgroup finishes
// the pull and runs the push down to that level again (a barrier between levels); the push of the finer levels is one launch per level.
// ------------------------------------------------------------------------------------------------------------------
struct ReconTexel { float v[7]; float w; };

__device__ __forceinline__ bool recon_attempt_void(const ReconParams& C) { return C.words[0] > C.sub_capacity; }
__device__ __forceinline__ bool recon_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ ReconTexel recon_zero()
{
  ReconTexel t;
#pragma unroll
  for (int c = 0; c < 7; ++c) t.v[c] = 0.f;
  t.w = 0.f;
  return t;
}

// level 0: v0 and w0 of pixel (x, y), n = N(p); a pixel outside the image or without a sample reads as an invalid child
__device__ __forceinline__ ReconTexel recon_load0(const ReconParams& C, int x, int y, float& n)
{
  ReconTexel t = recon_zero();
  n = 0.f;
  if (x >= C.width || y >= C.height) return t;
  const size_t p = (size_t)x + (size_t)y * (size_t)C.width;
  n = C.count[p];
  if (!(n > 0.f)) return t;
  if (C.accum) {
    const float4 a = reinterpret_cast<const float4*>(C.accum)[p];
    t.v[0] = a.x / n; t.v[1] = a.y / n; t.v[2] = a.z / n; t.v[3] = a.w / n;
    if (C.grad) {
      const float* g = C.grad_sum + 3 * p;
      t.v[4] = g[0] / n; t.v[5] = g[1] / n; t.v[6] = g[2] / n;
    }
  }
  else {
    const float4 a = reinterpret_cast<const float4*>(C.rgba)[p];
    t.v[0] = a.x; t.v[1] = a.y; t.v[2] = a.z; t.v[3] = a.w;
    if (C.grad) {
      const float* g = C.grad + 3 * p;
      t.v[4] = g[0]; t.v[5] = g[1]; t.v[6] = g[2];
    }
  }
  bool finite = true;
#pragma unroll
  for (int c = 0; c < 7; ++c) finite = finite && recon_finite(t.v[c]);
  t.w = finite ? 1.f : 0.f;
  return t;
}

__device__ __forceinline__ float4* recon_texel_ptr(const ReconParams& C, int l, int x, int y)
{
  return C.pyramid + 2 * ((size_t)C.level_offset[l] + (size_t)x + (size_t)y * (size_t)C.level_w[l]);
}
__device__ __forceinline__ ReconTexel recon_load(const ReconParams& C, int l, int x, int y)
{
  if (x >= C.level_w[l] || y >= C.level_h[l]) return recon_zero();
  const float4* q = recon_texel_ptr(C, l, x, y);
  const float4 a = q[0], b = q[1];
  ReconTexel t;
  t.v[0] = a.x; t.v[1] = a.y; t.v[2] = a.z; t.v[3] = a.w; t.v[4] = b.x; t.v[5] = b.y; t.v[6] = b.z; t.w = b.w;
  return t;
}
__device__ __forceinline__ void recon_store(const ReconParams& C, int l, int x, int y, const ReconTexel& t)
{
  float4* q = recon_texel_ptr(C, l, x, y);
  q[0] = make_float4(t.v[0], t.v[1], t.v[2], t.v[3]);
  q[1] = make_float4(t.v[4], t.v[5], t.v[6], t.w);
}
__device__ __forceinline__ void recon_write_pixel(const ReconParams& C, int x, int y, const float v[7])
{
  const size_t p = (size_t)x + (size_t)y * (size_t)C.width;
  reinterpret_cast<float4*>(C.rgba)[p] = make_float4(v[0], v[1], v[2], v[3]);
  if (C.grad) {
    float* g = C.grad + 3 * p;
    g[0] = v[4]; g[1] = v[5]; g[2] = v[6];
  }
}

__global__ __launch_bounds__(256) void recon_scatter_kernel(const ReconParams C, float* count, float* grad_sum, const int32_t* __restrict__ list_xy,
                                                           const unsigned long long* __restrict__ list_count)
{
  if (recon_attempt_void(C)) return;
  const unsigned long long n = *list_count / 2ull;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull) {
    const int x = list_xy[2 * i], y = list_xy[2 * i + 1];
    if (x < 0 || y < 0 || x >= C.width || y >= C.height) continue;
    const size_t p = (size_t)x + (size_t)y * (size_t)C.width; // the list holds a pixel at most once: no atomics
    if (grad_sum) {
      count[p] += 1.f;
      if (C.grad) {
        const float* g = C.grad + 3 * p;
        float* s = grad_sum + 3 * p;
        s[0] += g[0]; s[1] += g[1]; s[2] += g[2];
      }
    }
    else count[p] = 1.f;
  }
}

// levels src + 1 ... src + nlev (nlev <= 3) from level src: one wave per 8x8 block of level src
__global__ __launch_bounds__(256) void recon_pull_kernel(const ReconParams C, int src, int nlev)
{
  if (recon_attempt_void(C)) return;
  const int bw = (C.level_w[src] + 7) >> 3, bh = (C.level_h[src] + 7) >> 3;
  const unsigned int b = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (b >= (unsigned int)bw * (unsigned int)bh) return; // wave-uniform
  const int lane = threadIdx.x & 63, lx = lane & 7, ly = lane >> 3;
  const int x = (int)(b % (unsigned int)bw) * 8 + lx, y = (int)(b / (unsigned int)bw) * 8 + ly;
  ReconTexel t;
  if (src == 0) {
    float n;
    t = recon_load0(C, x, y, n);
    const unsigned int sampled = (unsigned int)__popcll(__ballot(n > 0.f));
    if (lane == 0 && sampled > 0u) atomicAdd(&C.words[2 + (b & 63u)], sampled); // (64 words: the waves of a frame do not queue on one address)
  }
  else t = recon_load(C, src, x, y);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k >= nlev) break;
    const int ox = 1 << k, oy = 8 << k;
    float s = t.w + __shfl_xor(t.w, ox);
    s = s + __shfl_xor(s, oy);
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      float u = t.w == 1.f ? t.v[c] : 0.f;
      u = u + __shfl_xor(u, ox);
      u = u + __shfl_xor(u, oy);
      t.v[c] = s > 0.f ? u / s : 0.f;
    }
    t.w = s > 0.f ? 1.f : 0.f;
    const int l = src + k + 1, m = (2 << k) - 1, tx = x >> (k + 1), ty = y >> (k + 1);
    if ((lx & m) == 0 && (ly & m) == 0 && tx < C.level_w[l] && ty < C.level_h[l]) recon_store(C, l, tx, ty, t);
  }
}

// texel (x, y) of level l + 1 from its four children on level l
__device__ __forceinline__ void recon_pull_texel(const ReconParams& C, int l, int x, int y)
{
  ReconTexel c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float n;
    c[i] = l == 0 ? recon_load0(C, 2 * x + (i & 1), 2 * y + (i >> 1), n) : recon_load(C, l, 2 * x + (i & 1), 2 * y + (i >> 1));
  }
  const float s = (c[0].w + c[1].w) + (c[2].w + c[3].w);
  ReconTexel t;
#pragma unroll
  for (int ch = 0; ch < 7; ++ch) {
    const float u0 = c[0].w == 1.f ? c[0].v[ch] : 0.f, u1 = c[1].w == 1.f ? c[1].v[ch] : 0.f;
    const float u2 = c[2].w == 1.f ? c[2].v[ch] : 0.f, u3 = c[3].w == 1.f ? c[3].v[ch] : 0.f;
    const float sum = (u0 + u1) + (u2 + u3);
    t.v[ch] = s > 0.f ? sum / s : 0.f;
  }
  t.w = s > 0.f ? 1.f : 0.f;
  recon_store(C, l + 1, x, y, t);
}

// U of texel (x, y) of level l: the bilinear interpolation of the completed level l + 1
__device__ __forceinline__ void recon_upsample(const ReconParams& C, int l, int x, int y, float U[7])
{
  const int lc = l + 1, wc = C.level_w[lc], hc = C.level_h[lc];
  const int px = x >> 1, py = y >> 1;
  const int nx = min(max(px + ((x & 1) ? 1 : -1), 0), wc - 1), ny = min(max(py + ((y & 1) ? 1 : -1), 0), hc - 1);
  const ReconTexel p00 = recon_load(C, lc, px, py), p10 = recon_load(C, lc, nx, py), p01 = recon_load(C, lc, px, ny), p11 = recon_load(C, lc, nx, ny);
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    const float a = 0.75f * p00.v[c] + 0.25f * p10.v[c];
    const float b = 0.75f * p01.v[c] + 0.25f * p11.v[c];
    U[c] = 0.75f * a + 0.25f * b;
  }
}

__device__ __forceinline__ void recon_push_texel(const ReconParams& C, int l, int x, int y) // l >= 1
{
  float4* q = recon_texel_ptr(C, l, x, y);
  if (q[1].w == 1.f) return; // a texel that has data keeps the mean of its sampled descendants
  float U[7];
  recon_upsample(C, l, x, y, U);
  q[0] = make_float4(U[0], U[1], U[2], U[3]);
  q[1] = make_float4(U[4], U[5], U[6], 0.f);
}

__device__ __forceinline__ void recon_push_pixel(const ReconParams& C, int x, int y)
{
  float n;
  const ReconTexel t = recon_load0(C, x, y, n);
  if (n > 0.f) { // a sampled pixel keeps its v0, finite or not; without accumulation that is what the framebuffer holds already
    if (C.accum) recon_write_pixel(C, x, y, t.v);
    return;
  }
  float U[7] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
  if (C.levels > 1) recon_upsample(C, 0, x, y, U);
  recon_write_pixel(C, x, y, U);
}

__global__ __launch_bounds__(256) void recon_push_kernel(const ReconParams C, int l)
{
  if (recon_attempt_void(C)) return;
  const int w = l == 0 ? C.width : C.level_w[l], h = l == 0 ? C.height : C.level_h[l];
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= (size_t)w * (size_t)h) return;
  const int x = (int)(i % (size_t)w), y = (int)(i / (size_t)w);
  if (l == 0) recon_push_pixel(C, x, y);
  else recon_push_texel(C, l, x, y);
}

// one workgroup: the pull from level `top` to the 1 x 1 level and the push back down to `top`, then the frame's counts for the host
__global__ __launch_bounds__(1024) void recon_top_kernel(const ReconParams C)
{
  if (recon_attempt_void(C)) return;
  const int tid = threadIdx.x;
  if (C.top == 0) { // (no pull pass counted the sampled pixels)
    unsigned int mine = 0u;
    for (int i = tid; i < C.width * C.height; i += 1024) mine += C.count[i] > 0.f ? 1u : 0u;
    if (mine > 0u) atomicAdd(&C.words[2 + (tid & 63)], mine);
  }
  for (int l = C.top; l + 1 < C.levels; ++l) {
    const int w = C.level_w[l + 1], n = w * C.level_h[l + 1];
    for (int i = tid; i < n; i += 1024) recon_pull_texel(C, l, i % w, i / w);
    __syncthreads();
  }
  for (int l = C.levels - 1; l >= C.top; --l) {
    if (l >= 1 && l == C.levels - 1) continue; // the 1 x 1 level is complete as it is
    const int w = C.level_w[l], n = w * C.level_h[l];
    for (int i = tid; i < n; i += 1024) {
      if (l == 0) recon_push_pixel(C, i % w, i / w);
      else recon_push_texel(C, l, i % w, i / w);
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid < 64) {
    unsigned int v = __hip_atomic_load(&C.words[2 + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    C.words[2 + tid] = 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned int)__shfl_xor((int)v, off);
    if (tid == 0 && C.publish) { C.publish[0] = v; C.publish[1] = (unsigned int)C.frame_index; }
  }
}

size_t recon_plan(ReconParams& c)
{
  int w = c.width, h = c.height, l = 0;
  size_t texels = 0;
  c.top = -1;
  for (;; ++l) {
    c.level_w[l] = w; c.level_h[l] = h;
    c.level_offset[l] = l == 0 ? 0u : (unsigned int)texels;
    if (l >= 1) texels += (size_t)w * (size_t)h;
    if (c.top < 0 && w <= 64 && h <= 64) c.top = l;
    if ((w <= 1 && h <= 1) || l + 1 >= kReconMaxLevels) break;
    w = (w + 1) / 2; h = (h + 1) / 2;
  }
  c.levels = l + 1;
  return texels;
}

int recon_launch_count(const ReconParams& c) { return (c.top + 2) / 3 + 1 + c.top; }

hipError_t launch_recon_scatter(const ReconParams& c, float* count, float* grad_sum, const int32_t* list_xy, const unsigned long long* list_count, hipStream_t stream)
{
  const size_t blocks = std::min<size_t>(((size_t)c.width * (size_t)c.height + 255) / 256, 2048);
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(recon_scatter_kernel, dim3((unsigned int)blocks), dim3(256), 0, stream, c, count, grad_sum, list_xy, list_count);
  return hipGetLastError();
}

hipError_t launch_reconstruct(const ReconParams& c, hipStream_t stream)
{
  if (c.width <= 0 || c.height <= 0 || c.levels <= 0 || c.top < 0) return hipErrorInvalidValue;
  for (int src = 0; src < c.top;) {
    const int nlev = std::min(3, c.top - src);
    const unsigned int blocks = (unsigned int)((c.level_w[src] + 7) / 8) * (unsigned int)((c.level_h[src] + 7) / 8);
    hipLaunchKernelGGL(recon_pull_kernel, dim3((blocks + 3u) / 4u), dim3(256), 0, stream, c, src, nlev);
    src += nlev;
  }
  hipLaunchKernelGGL(recon_top_kernel, dim3(1), dim3(1024), 0, stream, c);
  for (int l = c.top - 1; l >= 0; --l) {
    const size_t n = (size_t)c.level_w[l] * (size_t)c.level_h[l];
    hipLaunchKernelGGL(recon_push_kernel, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, stream, c, l);
  }
  return hipGetLastError();
}

static_assert(kCounterWords == kBlockCounters && axis_a_entries(0) + axis_b_entries(0) == kAxisAbExtra && axis_z_entries(0) == kAxisZExtra
                && axis_a_entries(7) + axis_b_entries(9) == 7 + 9 + kAxisAbExtra && axis_z_entries(5) == 5 + kAxisZExtra,
              "launch_plan.hpp restates ovr_hip_kernels.h: the counters of a workgroup and the entries of the axis tables that stage_tables copies into LDS");
size_t raymarch_lds_bytes(int n_color, int n_alpha) { return tf_lds_bytes(n_color, n_alpha); }

int volume_addressing_mode(const VolumeDesc& vd, int n_color, int n_alpha)
{
  return addressing_mode(vd.bytes, (int)voxel_size(vd.type), vd.nx, vd.ny, vd.nz, n_color, n_alpha);
}

size_t raymarch_grid_blocks(const RayMarchParams& p)
{
  if (p.sparse_xy) return ((size_t)p.width * p.height + kBlock / 4 - 1) / (kBlock / 4);
  return p.n_schedule;
}

static hipError_t launch_composite(const RayMarchParams& q, dim3 grid, hipStream_t stream)
{
  hipLaunchKernelGGL(composite_kernel, grid, dim3(kBlock), 0, stream, q);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// shade order by light beams (PoolDesc): the march has left a key per run and the histogram of the keys; every workgroup scans
// the histogram in LDS (G*G entries, the same result everywhere), then a thread per run slot writes its run to its place
// ------------------------------------------------------------------------------------------------------------------
constexpr int kOrderSlots = 4; // run slots per thread of the order kernel
__global__ __launch_bounds__(256) void shade_order_kernel(const RayMarchParams P)
{
  extern __shared__ __attribute__((aligned(16))) unsigned int s_off[]; // G*G exclusive offsets
  __shared__ unsigned int s_wave[4];
  const PoolDesc& Q = P.pool;
  const int n = Q.order_grid * Q.order_grid; // 1024, 4096 or 16384 keys
  // each wave scans a contiguous quarter, 256 entries (one uint4 per lane) at a time, four loads in flight
  const int it = n / 1024;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint4* h4 = reinterpret_cast<const uint4*>(Q.order_ws + kOrderHist) + wave * (n / 16);
  uint4* o4 = reinterpret_cast<uint4*>(s_off) + wave * (n / 16);
  unsigned int carry = 0;
  for (int g = 0; g < it; g += 4) {
    uint4 h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = (g + k < it) ? h4[(g + k) * 64 + lane] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (g + k < it) {
        const unsigned int sum = h[k].x + h[k].y + h[k].z + h[k].w;
        unsigned int incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const unsigned int t = __shfl_up(incl, off);
          if (lane >= off) incl += t;
        }
        const unsigned int ex = carry + incl - sum;
        o4[(g + k) * 64 + lane] = make_uint4(ex, ex + h[k].x, ex + h[k].x + h[k].y, ex + h[k].x + h[k].y + h[k].z);
        carry += __shfl(incl, 63);
      }
  }
  if (lane == 0) s_wave[wave] = carry;
  __syncthreads();
  unsigned int base = 0;
  for (int w = 0; w < wave; ++w) base += s_wave[w];
  if (wave > 0)
    for (int j = lane; j < n / 16; j += 64) {
      uint4 v = o4[j];
      v.x += base; v.y += base; v.z += base; v.w += base;
      o4[j] = v;
    }
  __syncthreads();
  if (blockIdx.x == 0) { // the lists' bounds and their ticket counters
    if (threadIdx.x < (unsigned int)kOrderLists) {
      Q.order_ws[kOrderListStart + threadIdx.x] = s_off[threadIdx.x * (n / kOrderLists)];
      Q.order_ws[kOrderTickets + 32 * threadIdx.x] = 0u;
    }
    if (threadIdx.x == 255) Q.order_ws[kOrderListStart + kOrderLists] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  }
  const unsigned int rps = Q.sub_capacity / (unsigned int)kRun, slots = rps * (unsigned int)kPoolSubs; // run slots per sub-pool / of the pool
  // kOrderSlots run slots per thread, their keys loaded together (the chain key -> fill counter -> order entry is all latency)
  unsigned int key[kOrderSlots], gid[kOrderSlots];
#pragma unroll
  for (int k = 0; k < kOrderSlots; ++k) {
    gid[k] = (blockIdx.x * (unsigned int)kOrderSlots + (unsigned int)k) * 256u + threadIdx.x;
    key[k] = kOrderNoKey;
    if (gid[k] < slots) {
      const unsigned int sub = gid[k] / rps, run = gid[k] - sub * rps;
      if (run < min(Q.ctrl[32u * (sub + 1u)], Q.sub_capacity) / (unsigned int)kRun) key[k] = Q.order_key[gid[k]]; // reserved in this generation
    }
  }
#pragma unroll
  for (int k = 0; k < kOrderSlots; ++k) {
    if (key[k] >= (unsigned int)n) continue; // kOrderNoKey: the unused tail of a reservation
    const unsigned int pos = s_off[key[k]] + atomicAdd(&Q.order_ws[kOrderFill + key[k]], 1u);
    if (pos < slots) Q.order[pos] = gid[k]; // (always, unless a launch was lost between a march and its shade kernel)
  }
}

// every launch with dynamic LDS: one needing 64 KiB of it or more raises the kernel's limit first (from 64 KiB: a kernel's static words count against the same
// limit; per launch: the attribute belongs to the current device's copy of the kernel).  An empty grid launches nothing
template <typename... Params, typename... Args>
static hipError_t launch_variant(void (*kern)(Params...), dim3 grid, int block, size_t lds, hipStream_t stream, const Args&... args)
{
  if (lds >= 64 * 1024)
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  if (grid.x > 0) hipLaunchKernelGGL(kern, grid, dim3(block), lds, stream, static_cast<Params>(args)...);
  return hipGetLastError();
}

static hipError_t launch_shade_order(const RayMarchParams& q, hipStream_t stream)
{
  const unsigned int slots = q.pool.capacity / (unsigned int)kRun;
  const dim3 grid((slots + 256u * kOrderSlots - 1u) / (256u * kOrderSlots));
  if (grid.x == 0) return hipSuccess;
  return launch_variant(shade_order_kernel, grid, 256, (size_t)q.pool.order_grid * q.pool.order_grid * sizeof(unsigned int), stream, q); // (128 x 128 beams: 64 KiB of offsets)
}

constexpr int kReduceBlocks = 64;
static hipError_t launch_reduce_counters(const unsigned int* partials, int n_blocks, const unsigned int* shade_partials, int n_shade_blocks,
                                         unsigned long long* counters, unsigned int* pool_ctrl, unsigned long long* publish, unsigned int* done, hipStream_t stream,
                                         unsigned int* conv_asked)
{
  hipLaunchKernelGGL(reduce_counters_kernel, dim3(kReduceBlocks), dim3(256), 0, stream, partials, n_blocks, shade_partials, n_shade_blocks, counters, pool_ctrl,
                     done ? publish : nullptr, done, conv_asked);
  return hipGetLastError();
}

size_t pool_shade_blocks() { return kShadeBlocks; }

// the facts of a frame's launch, and the environment switches: OVR_HIP_ADDRESSING=k is read with every plan (a more general addressing mode than needed:
// tests change it between renderers), OVR_HIP_DEEP=0|1 and OVR_HIP_SHADE_BLOCKS=n once per process (measurements)
LaunchPlan plan_raymarch(const RayMarchParams& p)
{
  static const int deep = getenv("OVR_HIP_DEEP") ? atoi(getenv("OVR_HIP_DEEP")) : -1;
  static const int shade_blocks = getenv("OVR_HIP_SHADE_BLOCKS") ? atoi(getenv("OVR_HIP_SHADE_BLOCKS")) : 0;
  LaunchOverrides o;
  if (const char* a = getenv("OVR_HIP_ADDRESSING")) o.addressing = atoi(a);
  o.deep = deep;
  o.shade_blocks = shade_blocks;
  LaunchFacts f;
  f.elem_bytes = (int)voxel_size(p.vol.type);
  f.quad = p.vol.type >= 0 && p.vol.type < kVoxelTypeCount && kVoxelTypes[p.vol.type].layout == LAYOUT_QUAD;
  f.f32_general = p.vol.type == VOX_F32;
  f.nx = p.vol.nx; f.ny = p.vol.ny; f.nz = p.vol.nz;
  f.stored_bytes = p.vol.bytes;
  f.tables = p.vol.axis_ab && p.vol.axis_z;
  f.n_color = p.n_color; f.n_alpha = p.n_alpha; f.shading = p.shading;
  f.pool = p.pool.reqs != nullptr; f.skipping = p.majorant != nullptr; f.sparse = p.sparse_xy != nullptr;
  f.sparse_hint_pixels = p.sparse_hint_pixels;
  f.world = p.world;
  f.n_blocks_owned = p.n_blocks_owned; f.n_schedule = p.n_schedule; f.schedule = p.schedule != nullptr;
  f.clip_on = p.clip_on != 0; f.lds_staging = p.lds_staging != 0;
  f.row_loads = p.row_loads; f.shade_blocks = p.shade_blocks;
  f.reference_material = reference_material(p); f.shade_order = p.pool.order != nullptr;
  f.shadow_cache = p.shadow_lattice != nullptr;
  f.projection = p.projection; f.ranges = p.mc_ranges != nullptr;
  f.isosurfaces = p.iso_n;
  f.translucent = p.iso_n > 0 && p.iso_translucent != 0;
  f.ambient_occlusion = p.iso_n > 0 && p.ao_samples > 0;
  f.orthographic = p.cam_orthographic != 0;
  f.slices = p.slice_n;
  for (int k = 0; k < p.slice_n && k < kMaxSlices; ++k) {
    f.slice_walks = f.slice_walks || p.slice_mode[k] != 0;
    f.slice_extremum = f.slice_extremum || p.slice_mode[k] == kProjectMaximum || p.slice_mode[k] == kProjectMinimum;
  }
  f.slice_context = p.slice_n > 0 && p.slice_context != 0;
  f.isosurface_context = p.iso_n > 0 && p.iso_context != 0;
  f.preintegrated = p.preintegrated != 0;
  f.gradient_opacity = p.gradient_opacity != 0;
  f.max_depth = p.max_depth != nullptr;
  f.depth_output = p.depth_tau > 0.f;
  f.depth_threshold = p.depth_tau;
  return plan_launch(f, o);
}

// the frame's kernels between its first and last event: in place march -> reduction; pooled, once per sample-per-pixel generation,
// march -> (order) -> shade -> composite -> reduction
static hipError_t launch_sequence(const RayMarchParams& p, const LaunchPlan& plan, const FrameKernels& k, hipStream_t stream, const hipEvent_t* ev)
{
  const dim3 grid((unsigned)raymarch_grid_blocks(p)); // (no march or composite workgroup when no block of this renderer's has a hit)
  hipError_t e;
  if (!plan.pooled) {
    RayMarchParams q = p;
    if (plan.march.lds_staged) q.lds_brick_offset = plan.lds_brick_offset; // the bricks follow the tables and the TF
    if ((e = launch_variant(k.march, grid, kBlock, plan.march_lds_bytes, stream, q)) != hipSuccess) return e;
    if (ev && ev[1] && ev[2]) { (void)hipEventRecord(ev[1], stream); (void)hipEventRecord(ev[2], stream); }
    if (p.block_counters && p.counters) {
      if (!p.publish || p.zero_first)
        if ((e = hipMemsetAsync(p.counters, 0, 8 * sizeof(unsigned long long), stream)) != hipSuccess) return e;
      if ((e = launch_reduce_counters(p.block_counters, (int)grid.x, nullptr, 0, p.counters, nullptr, p.publish, p.reduce_done, stream, p.conv_asked)) != hipSuccess) return e;
    }
    return hipGetLastError();
  }
  // (the last frame's final reduction left the control words and the counters zeroed - RayMarchParams::publish)
  const bool self_cleaning = p.publish && p.block_counters && p.counters && !p.zero_first;
  if (!self_cleaning) {
    if ((e = hipMemsetAsync(p.pool.ctrl, 0, (size_t)kPoolCtrlWords * sizeof(unsigned int), stream)) != hipSuccess) return e;
    if (p.block_counters && p.counters)
      if ((e = hipMemsetAsync(p.counters, 0, 8 * sizeof(unsigned long long), stream)) != hipSuccess) return e;
  }
  RayMarchParams q = p;
  if (!plan.shade_order) q.pool.order = nullptr;
  for (int g = 0; g < p.spp; ++g) {
    q.spp_index = g;
    if (g > 0 && (e = hipMemsetAsync(p.pool.ctrl, 0, (size_t)32 * (kPoolSubs + 1) * sizeof(unsigned int), stream)) != hipSuccess) return e; // all but the frame's maximum
    if ((e = launch_variant(k.march, grid, kBlock, plan.march_lds_bytes, stream, q)) != hipSuccess) return e;
    if (ev && ev[1] && g == p.spp - 1) (void)hipEventRecord(ev[1], stream);
    if (q.pool.order && (e = launch_shade_order(q, stream)) != hipSuccess) return e; // runs sorted by light beam (PoolDesc)
    if ((e = launch_variant(k.shade, dim3((unsigned)plan.shade_grid_blocks), kBlock, plan.shade_lds_bytes, stream, q)) != hipSuccess) return e;
    if (ev && ev[2] && g == p.spp - 1) (void)hipEventRecord(ev[2], stream);
    if (grid.x > 0 && (e = launch_composite(q, grid, stream)) != hipSuccess) return e;
    if (p.block_counters && p.counters)
      if ((e = launch_reduce_counters(p.block_counters, (int)grid.x, (const unsigned int*)p.pool.shade_counters, plan.shade_grid_blocks, p.counters, p.pool.ctrl,
                                      g == p.spp - 1 ? p.publish : nullptr, p.reduce_done, stream, p.conv_asked)) != hipSuccess) return e; // the frame's last generation publishes
  }
  return hipGetLastError();
}

// the lookups of ovr_hip_device.h, instantiated once per voxel type in objects of their own: ovr_hip_march.hip (every type), ovr_hip_isosurface.hip (the general
// layout's types alone, the opaque and the translucent kernels each in an object of their own - DESIGN.md section 19)
#define OVR_X(E, NAME, BASE, LAYOUT)                                                          \
  extern template FrameKernels frame_kernels<E>(const LaunchPlan&);                           \
  extern template ShadowCacheKernel shadow_cache_kernel_of<E>(int);                           \
  extern template ProjectKernels project_kernels_of<E>(const LaunchPlan&);                    \
  extern template IsosurfaceKernels isosurface_kernels_of<E, false>(const LaunchPlan&);       \
  extern template IsosurfaceLayersKernels isosurface_kernels_of<E, true>(const LaunchPlan&);
#define OVR_X_AO(E, NAME, BASE, LAYOUT) extern template IsosurfaceAoKernels isosurface_ao_kernels_of<E>(const LaunchPlan&);
#define OVR_X_SLICES(E, NAME, BASE, LAYOUT)                                          \
  extern template SliceKernels slice_kernels_of<E>(const LaunchPlan&);               \
  extern template SliceContextKernels slice_context_kernels_of<E>(const LaunchPlan&); \
  extern template IsosurfaceContextKernels isosurface_context_kernels_of<E>(const LaunchPlan&); \
  extern template PreintegratedKernels preintegrated_kernels_of<E>(const LaunchPlan&); \
  extern template GradientOpacityKernels gradient_opacity_kernels_of<E>(const LaunchPlan&); \
  extern template MaxDepthKernels max_depth_kernels_of<E>(const LaunchPlan&); \
  extern template DepthOutputKernels depth_output_kernels_of<E>(const LaunchPlan&);
OVR_VOXEL_TYPES(OVR_X)
OVR_VOXEL_TYPES(OVR_X_AO)
OVR_VOXEL_TYPES(OVR_X_SLICES)
#undef OVR_X
#undef OVR_X_AO
#undef OVR_X_SLICES

// a plan's kernels for the volume's voxel type: the frame's two - the kernel of another frame kind in the in-place march's place (such a plan is neither pooled nor
// LDS-staged, march_lds_bytes is that kernel's) - and the known-answer twin of such a kernel, filed by its signature: launch_ray_query holds the plan's kind to
// the query's before it calls one.  All nullptr: the plan is an error, or no such variant
typedef void (*QueryKernel)(const RayMarchParams, const float*, const float*, float*, long long);
typedef void (*QueryEventsKernel)(const RayMarchParams, const float*, const float*, float*, long long, int);        // + max_events
typedef void (*QueryRotationKernel)(const RayMarchParams, const float*, const float*, float*, long long, int, int); // + max_events, rotation
typedef void (*QueryDepthKernel)(const RayMarchParams, const float*, const float*, const float*, float*, long long); // + one ray parameter per ray, behind dir
struct PlanKernels {
  FrameKernels frame;
  QueryKernel query = nullptr;
  QueryEventsKernel query_events = nullptr;
  QueryRotationKernel query_rotation = nullptr;
  QueryDepthKernel query_depth = nullptr;
  void set(QueryKernel k) { query = k; }
  void set(QueryEventsKernel k) { query_events = k; }
  void set(QueryRotationKernel k) { query_rotation = k; }
  void set(QueryDepthKernel k) { query_depth = k; }
  template <typename V> void take(const V& v) { frame.march = v.frame; set(v.floats); } // (the pair a *_kernels_of lookup returns)
};
static PlanKernels plan_kernels(const RayMarchParams& p, const LaunchPlan& plan)
{
  PlanKernels k;
  if (plan.error) return k;
  const int t = p.vol.type;
  switch (frame_kind(plan)) {
  case FrameKind::SliceContext: dispatch_voxel_type<true>(t, [&](auto vt) { k.take(slice_context_kernels_of<decltype(vt)::value>(plan)); }); break;
  case FrameKind::SlicePlane:
  case FrameKind::SliceWalk: dispatch_voxel_type<true>(t, [&](auto vt) { k.take(slice_kernels_of<decltype(vt)::value>(plan)); }); break;
  case FrameKind::IsosurfaceContext: dispatch_voxel_type<true>(t, [&](auto vt) { k.take(isosurface_context_kernels_of<decltype(vt)::value>(plan)); }); break;
  case FrameKind::IsosurfaceAo:
    if (p.ao_dirs && p.ao_samples > 0 && p.ao_samples <= kAoMaxSamples) // (the AO kernels read the direction table: no table, no kernel)
      dispatch_voxel_type<true>(t, [&](auto vt) { k.take(isosurface_ao_kernels_of<decltype(vt)::value>(plan)); });
    break;
  case FrameKind::IsosurfaceLayers: dispatch_voxel_type<true>(t, [&](auto vt) { k.take(isosurface_kernels_of<decltype(vt)::value, true>(plan)); }); break;
  case FrameKind::Isosurface: dispatch_voxel_type<true>(t, [&](auto vt) { k.take(isosurface_kernels_of<decltype(vt)::value, false>(plan)); }); break;
  case FrameKind::Projection: dispatch_voxel_type(t, [&](auto vt) { k.take(project_kernels_of<decltype(vt)::value>(plan)); }); break;
  case FrameKind::PreintegratedMarch:
    if (p.preint_nodes && p.preint_m1 == plan.preintegrated.nodes - 1) // (the kernels stage the node table the plan sized its LDS for: no table, no kernel)
      dispatch_voxel_type<true>(t, [&](auto vt) { k.take(preintegrated_kernels_of<decltype(vt)::value>(plan)); });
    break;
  case FrameKind::GradientOpacityMarch: dispatch_voxel_type<true>(t, [&](auto vt) { k.take(gradient_opacity_kernels_of<decltype(vt)::value>(plan)); }); break;
  case FrameKind::DepthLimitedMarch:
    if (p.max_depth) // (the kernel loads the pixel's depth: no image, no kernel)
      dispatch_voxel_type<true>(t, [&](auto vt) { k.take(max_depth_kernels_of<decltype(vt)::value>(plan)); });
    break;
  case FrameKind::DepthOutputMarch: // (a null image is no limit: the kernel takes z = +inf without a load)
    dispatch_voxel_type<true>(t, [&](auto vt) { k.take(depth_output_kernels_of<decltype(vt)::value>(plan)); });
    break;
  case FrameKind::March: dispatch_voxel_type(t, [&](auto vt) { k.frame = frame_kernels<decltype(vt)::value>(plan); }); break;
  }
  return k;
}

hipError_t launch_raymarch(const RayMarchParams& p, const LaunchPlan& plan, hipStream_t stream, const hipEvent_t* ev)
{
  // ev (optional): ev[0] before the first kernel, ev[1] after the march, ev[2] after the shade kernel (both may be null: no per-phase times), ev[3] at the end
  if (ev) (void)hipEventRecord(ev[0], stream);
  const FrameKernels k = plan_kernels(p, plan).frame; // (a projection or an isosurface frame: the same reduction and publish steps behind its kernel)
  const hipError_t e = k.march && (k.shade || !plan.pooled) ? launch_sequence(p, plan, k, stream, ev) : hipErrorInvalidValue;
  if (ev) (void)hipEventRecord(ev[3], stream);
  return e;
}

// ------------------------------------------------------------------------------------------------------------------
// volume relayout: linear (x fastest) -> 128-byte x-apron bricks in macro blocks
// ------------------------------------------------------------------------------------------------------------------
// the reference's ValueType -> (input scalar TI, stored scalar TO, general VoxelType VT): u32 / i32 -> normalized f32, f64 -> f32 at upload.
// f(ValueTypeOf<..>{}); false - and f not called - for an unknown ValueType
template <typename TI_, int VT_> struct ValueTypeOf { typedef TI_ TI; typedef typename Vox<VT_>::T TO; static constexpr int VT = VT_; };
template <typename F>
static bool dispatch_value_type(int ovr_value_type, F&& f)
{
  switch (ovr_value_type) {
  case 100: f(ValueTypeOf<unsigned char, VOX_U8>{}); return true;
  case 101: f(ValueTypeOf<signed char, VOX_I8>{}); return true;
  case 200: f(ValueTypeOf<unsigned short, VOX_U16>{}); return true;
  case 201: f(ValueTypeOf<short, VOX_I16>{}); return true;
  case 300: f(ValueTypeOf<unsigned int, VOX_F32>{}); return true;
  case 301: f(ValueTypeOf<int, VOX_F32>{}); return true;
  case 400: f(ValueTypeOf<float, VOX_F32>{}); return true;
  case 500: f(ValueTypeOf<double, VOX_F32>{}); return true;
  default: return false;
  }
}
int device_voxel_type(int t)
{
  int vt = -1;
  dispatch_value_type(t, [&](auto v) { vt = decltype(v)::VT; });
  return vt;
}
size_t voxel_size(int vt)
{
  size_t bytes = 4;
  dispatch_voxel_type(vt, [&](auto t) { bytes = sizeof(typename Vox<decltype(t)::value>::T); });
  return bytes;
}

template <typename TI, typename TO> struct Conv { static __device__ __forceinline__ TO cv(TI v) { return (TO)v; } };
template <> struct Conv<unsigned int, float> { // integer_normalize<float, uint32_t>, array.h:68-76
  static __device__ __forceinline__ float cv(unsigned int v) { return (float)v / (float)0xffffffffu; }
};
template <> struct Conv<int, float> { // array.h:78-90
  static __device__ __forceinline__ float cv(int v) { const float n = (float)v / (float)0x7fffffff; return n < -1.f ? -1.f : n; }
};

// where a relayout kernel reads voxel (x, y, z) from: the caller's linear array (x fastest; slices [z0, z0 + nz_chunk) of it), or the
// resident GENERAL layout of the same volume (replicas built in the background, round 4: every replica is a permutation of the general layout's voxels)
template <typename TI> struct SrcLinear {
  typedef TI value_type;
  static constexpr bool kLinear = true;
  const TI* p; int nx, ny, z0;
  __device__ __forceinline__ TI get(size_t x, size_t y, unsigned z) const { return p[x + (size_t)nx * (y + (size_t)ny * (size_t)(z - (unsigned)z0))]; }
};
template <int VTB> struct SrcBricked {
  typedef typename Vox<VTB>::T value_type;
  static constexpr bool kLinear = false;
  static constexpr bool kBox = false;
  const value_type* p; unsigned int macro_y; unsigned long long macro_z;
  __device__ __forceinline__ value_type get(size_t x, size_t y, unsigned z) const
  {
    typedef BrickMap<VTB> M;
    return p[(unsigned long long)(M::X((unsigned)x + 1u) + M::Y((unsigned)y, macro_y)) + M::Zlo(z) + (unsigned long long)(z >> 5) * macro_z];
  }
};
template <int VTB> static SrcBricked<VTB> src_bricked(const VolumeDesc& general)
{
  return SrcBricked<VTB>{ (const typename Vox<VTB>::T*)general.data, macro_stride_y(general), macro_stride_z(general) };
}

// One thread per brick ROW (the SX stored voxels of one (y, z) line of a brick: 8 or 16 bytes), rows taken in the order the layout stores them:
// a workgroup owns the 32 y x 2^bz z slab of one macro row and sweeps it along the pair axis, macro block by macro block - inside a macro block
// that slab is ONE contiguous piece of the layout ((32 >> by) * mbx bricks, 10 KiB for f32), so consecutive lanes store consecutive vectors and
// every 128-byte line leaves the workgroup complete.  (Until round 4 a thread was one stored voxel and a workgroup one source row: a 16-byte
// piece of every line per workgroup, the rest of the line from 7 other workgroups on other XCDs - 8.8 ms for C3's 10 GB, 0.14 of the HBM peak.)
// The source rows of the slab (64 for f32) are read in step along x: each line of the caller's array is fetched once and used up within the workgroup.
template <typename TI, int N> struct __attribute__((packed, aligned(sizeof(TI)))) RowIn { TI v[N]; };
template <typename TO, int N> struct alignas(sizeof(TO) * N) RowOut { TO v[N]; };

// The addressing of that sweep, shared by relayout_kernel and its box-restricted sibling update_rows_kernel (an update has to reproduce a fresh
// upload bit for bit).  layout axes (a, b, z): a = pair axis = x (y in a transposed replica), b = the other one.
// (The clamped gather of a row stays written out in both kernels: as a function the compiler simplifies it before it is inlined, without the
// caller's v0, and every kernel's instructions change - profiles/r11_voxel_types.md.)
template <int VT> struct RowSweep {
  typedef BrickMap<VT> M;
  typedef Vox<VT> V;
  static constexpr unsigned SX = M::SX, RB = 1u << (V::by + V::bz);   // stored voxels per row, rows per brick
  static constexpr unsigned ROWS = M::sbz / SX;                        // rows of the slab inside one macro block
  static constexpr unsigned LZ = 32u >> V::bz;                         // z layers per macro block
  static_assert(ROWS * SX == M::sbz && ROWS == (32u >> V::by) * V::mbx * RB, "the slab is the layout's z-layer stride");
  // element offset of the slab of (macro row my, z layer)
  static __device__ __forceinline__ unsigned long long slab(unsigned my, unsigned layer, unsigned int macro_y, unsigned long long macro_z)
  {
    return (unsigned long long)my * macro_y + (unsigned long long)(layer & (LZ - 1u)) * M::sbz + (unsigned long long)(layer / LZ) * macro_z;
  }
  // sweep index g (of a sweep that starts at macro block macro_lo) -> macro block along a, row in the slab, the row's b and z, its brick along a
  // (the row's stored positions br * cx ... br * cx + SX - 1 = voxels br * cx - 1 ...: clamp addressing is baked into the data, position 0 is a
  // copy of voxel 0, positions beyond the grid replicate the last voxel)
  struct Row { unsigned mx, i, b, z, br; };
  static __device__ __forceinline__ Row decode(unsigned g, unsigned macro_lo, unsigned my, unsigned layer)
  {
    const unsigned ml = g / ROWS, i = g - ml * ROWS, mx = macro_lo + ml;
    const unsigned rr = i & (RB - 1u), bi = i / RB;
    const unsigned ybk = bi / V::mbx, bm = bi - ybk * V::mbx;
    const unsigned b = my * 32u + (ybk << V::by) + (rr & ((1u << V::by) - 1u));
    const unsigned z = (layer << V::bz) + (rr >> V::by);
    return Row{ mx, i, b, z, mx * V::mbx + bm };
  }
  template <typename TO> static __device__ __forceinline__ RowOut<TO, SX>* row(TO* dst, unsigned long long slab_offset, const Row& r)
  {
    return reinterpret_cast<RowOut<TO, SX>*>(dst + slab_offset + (unsigned long long)r.mx * M::MV) + r.i;
  }
};

template <typename SRC, typename TO, int VT>
__global__ __launch_bounds__(256) void relayout_kernel(const SRC src, TO* __restrict__ dst, int nx, int ny, int macros_a, unsigned int macro_y,
                                                      unsigned long long macro_z, int z0, int nz_chunk, int nz)
{
  typedef typename SRC::value_type TI;
  // grid: x = macro rows along b, y = z layers (2^bz slices each) that meet [z0, z0 + nz_chunk) - and, in the launch of the volume's last
  // slices, the padding layers up to the end of the allocation ; src holds slices [z0, z0 + nz_chunk)
  typedef RowSweep<VT> S;
  typedef Vox<VT> V;
  constexpr bool TR = V::kTransposed;
  constexpr unsigned SX = S::SX;
  const int na = TR ? ny : nx, nb = TR ? nx : ny;
  const unsigned my = blockIdx.x, layer = ((unsigned)z0 >> V::bz) + blockIdx.y;
  const unsigned long long slab = S::slab(my, layer, macro_y, macro_z);
  const unsigned total = (unsigned)macros_a * S::ROWS;
  for (unsigned g = threadIdx.x; g < total; g += 256u) {
    const typename S::Row r = S::decode(g, 0u, my, layer);
    const unsigned b = r.b, z = r.z;
    RowOut<TO, SX>* const row = S::row(dst, slab, r);
    if (b >= (unsigned)nb || z >= (unsigned)nz) { // a padding row: never sampled, but finite (the allocation needs no memset)
      if (z >= (unsigned)z0) {                    // ... written once: by the launch whose slices the row's layer belongs to (or the last one)
        RowOut<TO, SX> zero;
#pragma unroll
        for (unsigned k = 0; k < SX; ++k) zero.v[k] = (TO)0;
        *row = zero;
      }
      continue;
    }
    if (z < (unsigned)z0 || z >= (unsigned)(z0 + nz_chunk)) continue; // another launch's slices
    const int v0 = (int)(r.br * V::cx) - 1;
    TI in[SX];
    bool done = false;
    if constexpr (SRC::kLinear && !TR) {
      if (v0 >= 0 && v0 + (int)SX <= nx) { // the whole row lies inside the grid: one (unaligned) vector load
        const RowIn<TI, SX> w = *reinterpret_cast<const RowIn<TI, SX>*>(src.p + ((size_t)v0 + (size_t)nx * ((size_t)b + (size_t)ny * (size_t)(z - (unsigned)z0))));
#pragma unroll
        for (unsigned k = 0; k < SX; ++k) in[k] = w.v[k];
        done = true;
      }
    }
    if (!done) {
#pragma unroll
      for (unsigned k = 0; k < SX; ++k) {
        const size_t as = (size_t)min(max(v0 + (int)k, 0), na - 1);
        in[k] = TR ? src.get((size_t)b, as, z) : src.get(as, (size_t)b, z);
      }
    }
    RowOut<TO, SX> out;
#pragma unroll
    for (unsigned k = 0; k < SX; ++k) out.v[k] = Conv<TI, TO>::cv(in[k]);
    *row = out;
  }
}

// quad replicas: one thread per cell writes the cell's 2 x 2 (x, y) voxels of its z slice as one 4-vector, neighbours beyond the
// grid replaced by the last voxel (clamp-to-edge addressing).  Cells in storage order, like relayout_kernel's rows: a workgroup owns the
// 32 cells (y) x 2^lz slices slab of one macro row - inside a macro block one contiguous 32 KiB piece - and sweeps it along x, so every
// 128-byte line is written whole (the thread-per-cell-along-x form of round 3 built C3's 17 GB replica in 40 ms), padding cells as zeros.
// (the constants and the slab offset of that sweep, shared with the box-restricted sibling update_quad_kernel; the decode of the sweep index, the cell
// pointer and the cell's gather are written out in both: shared as RowSweep's are, they changed the kernels' instructions - profiles/r11_voxel_types.md)
template <int VT> struct QuadSweep {
  typedef BrickMap<VT> M;
  typedef Vox<VT> V;
  typedef typename V::T TO;
  typedef typename V::Q Q;
  static constexpr unsigned CB = 1u << (V::lx + V::ly + V::lz);          // cells per brick
  static constexpr unsigned LAYER = M::bx_ * M::by_ * M::BV;             // elements of one z layer (2^lz slices) of a macro block
  static constexpr unsigned CELLS = M::bx_ * M::by_ * CB;                // ... and its cells
  static constexpr unsigned LZ = 32u >> V::lz;
  static_assert(CB * 4u == M::BV && CELLS * 4u == LAYER, "a brick is CB cells of 4 elements");
  static __device__ __forceinline__ unsigned long long slab(unsigned my, unsigned layer, unsigned int macro_y, unsigned long long macro_z)
  {
    return (unsigned long long)my * macro_y + (unsigned long long)(layer & (LZ - 1u)) * LAYER + (unsigned long long)(layer / LZ) * macro_z;
  }
};
template <typename SRC, int VT>
__global__ __launch_bounds__(256) void relayout_quad_kernel(const SRC src, typename Vox<VT>::T* __restrict__ dst, int nx, int ny, int macros_x, unsigned int macro_y,
                                                           unsigned long long macro_z, int z0, int nz_chunk, int nz)
{
  typedef typename SRC::value_type TI;
  typedef QuadSweep<VT> S;
  typedef BrickMap<VT> M;
  typedef Vox<VT> V;
  typedef typename V::T TO;
  typedef typename V::Q Q;
  // grid: x = macro rows along y, y = z layers that meet [z0, z0 + nz_chunk) (+ the padding layers, in the launch of the last slices)
  const unsigned my = blockIdx.x, layer = ((unsigned)z0 >> V::lz) + blockIdx.y;
  const unsigned long long slab = S::slab(my, layer, macro_y, macro_z);
  const unsigned total = (unsigned)macros_x * S::CELLS;
  for (unsigned g = threadIdx.x; g < total; g += 256u) {
    const unsigned mx = g / S::CELLS, i = g - mx * S::CELLS;
    const unsigned j = i & (S::CB - 1u), brick = i / S::CB;
    // cell (u, v) = (x + 1, y + 1), x in [-1, nx - 1], y in [-1, ny - 1]
    const int u = (int)(mx * 32u + ((brick & (M::bx_ - 1u)) << V::lx) + (j & ((1u << V::lx) - 1u)));
    const int v = (int)(my * 32u + ((brick / M::bx_) << V::ly) + ((j >> V::lx) & ((1u << V::ly) - 1u)));
    const unsigned z = (layer << V::lz) + (j >> (V::lx + V::ly));
    Q* const cell = reinterpret_cast<Q*>(dst + slab + (unsigned long long)mx * M::MV + (unsigned long long)i * 4u);
    if (u > nx || v > ny || z >= (unsigned)nz) { // a padding cell: never sampled, but finite
      if (z >= (unsigned)z0) { Q zero; zero.x = zero.y = zero.z = zero.w = (TO)0; *cell = zero; }
      continue;
    }
    if (z < (unsigned)z0 || z >= (unsigned)(z0 + nz_chunk)) continue; // another launch's slices
    const int x = max(u - 1, 0), y = max(v - 1, 0);
    const int x1 = min(u, nx - 1), y1 = min(v, ny - 1);
    Q q;
    q.x = Conv<TI, TO>::cv(src.get((size_t)x, (size_t)y, z)); q.y = Conv<TI, TO>::cv(src.get((size_t)x1, (size_t)y, z));
    q.z = Conv<TI, TO>::cv(src.get((size_t)x, (size_t)y1, z)); q.w = Conv<TI, TO>::cv(src.get((size_t)x1, (size_t)y1, z));
    *cell = q;
  }
}
template <typename SRC, int VT>
static hipError_t relayout_quad_s(const SRC& src, void* dst, const VolumeDesc& vd, int z0, int nzc, hipStream_t stream)
{
  if (nzc <= 0) return hipSuccess;
  const unsigned last = z0 + nzc >= vd.nz ? (unsigned)vd.macros_z * (32u >> Vox<VT>::lz) - 1u : (unsigned)(z0 + nzc - 1) >> Vox<VT>::lz;
  dim3 grid((unsigned)vd.macros_y, last - ((unsigned)z0 >> Vox<VT>::lz) + 1u);
  hipLaunchKernelGGL((relayout_quad_kernel<SRC, VT>), grid, dim3(256), 0, stream, src, (typename Vox<VT>::T*)dst, vd.nx, vd.ny, vd.macros_x, macro_stride_y(vd),
                     macro_stride_z(vd), z0, nzc, vd.nz);
  return hipGetLastError();
}

template <typename SRC, typename TO, int VT>
static hipError_t relayout_s(const SRC& src, void* dst, const VolumeDesc& vd, int z0, int nzc, hipStream_t stream)
{
  if (nzc <= 0) return hipSuccess;
  // the launch of the volume's last slices also writes the padding layers behind them
  const unsigned last = z0 + nzc >= vd.nz ? (unsigned)vd.macros_z * (32u >> Vox<VT>::bz) - 1u : (unsigned)(z0 + nzc - 1) >> Vox<VT>::bz;
  const unsigned layers = last - ((unsigned)z0 >> Vox<VT>::bz) + 1u;
  dim3 grid((unsigned)vd.macros_y, layers);
  hipLaunchKernelGGL((relayout_kernel<SRC, TO, VT>), grid, dim3(256), 0, stream, src, (TO*)dst, vd.nx, vd.ny, vd.macros_x, macro_stride_y(vd), macro_stride_z(vd), z0, nzc,
                     vd.nz);
  return hipGetLastError();
}

// layout constants the host needs to size the allocation (vd.type, nx, ny, nz and the macro-block geometry of that layout)
template <int VT>
static void volume_layout_t(int nx, int ny, int nz, VolumeDesc& vd)
{
  typedef BrickMap<VT> M;
  const int na = Vox<VT>::kTransposed ? ny : nx, nb = Vox<VT>::kTransposed ? nx : ny;
  // the pair axis holds stored positions 0 ... na + 1 (voxel + 1; lower members 0 ... na); a quad replica has cells 0 ... n on both axes
  vd.macros_x = (na + 1 + (int)M::MCX - 1) / (int)M::MCX;
  vd.macros_y = ((Vox<VT>::kQuad ? nb + 1 : nb) + 31) / 32;
  vd.macros_z = (nz + 31) / 32;
  vd.macro_elems = M::MV;
  vd.bytes = (unsigned long long)vd.macros_x * vd.macros_y * vd.macros_z * M::MV * sizeof(typename Vox<VT>::T);
}
bool volume_layout(int voxel_type, int nx, int ny, int nz, VolumeDesc& vd)
{
  return dispatch_voxel_type(voxel_type, [&](auto vt) {
    vd.type = voxel_type;
    vd.nx = nx; vd.ny = ny; vd.nz = nz;
    volume_layout_t<decltype(vt)::value>(nx, ny, nz, vd);
  });
}

hipError_t launch_relayout(const void* src, int vt, void* dst, const VolumeDesc& vd, int z0, int nzc, hipStream_t stream)
{
  hipError_t e = hipErrorInvalidValue; // an unknown ValueType, or vd is not its general layout
  dispatch_value_type(vt, [&](auto v) {
    typedef decltype(v) V;
    typedef SrcLinear<typename V::TI> Src;
    if (vd.type == V::VT) e = relayout_s<Src, typename V::TO, V::VT>(Src{ (const typename V::TI*)src, vd.nx, vd.ny, z0 }, dst, vd, z0, nzc, stream);
  });
  return e;
}

// a replica from the resident general layout (the caller's array is gone by then: ovr_hip_set_volume does not keep it)
template <int VTB>
static hipError_t rebrick_b(const VolumeDesc& g, void* dst, const VolumeDesc& vd, int z0, int nzc, hipStream_t stream)
{
  typedef typename Vox<VTB>::T T;
  typedef SrcBricked<VTB> Src;
  constexpr int T1 = replica_voxel_type(VTB, LAYOUT_THIN), T2 = replica_voxel_type(VTB, LAYOUT_THIN_T), TQ = replica_voxel_type(VTB, LAYOUT_QUAD);
  if constexpr (TQ >= 0) { if (vd.type == TQ) return relayout_quad_s<Src, TQ>(src_bricked<VTB>(g), dst, vd, z0, nzc, stream); }
  if constexpr (T1 >= 0) { if (vd.type == T1) return relayout_s<Src, T, T1>(src_bricked<VTB>(g), dst, vd, z0, nzc, stream); }
  if constexpr (T2 >= 0) { if (vd.type == T2) return relayout_s<Src, T, T2>(src_bricked<VTB>(g), dst, vd, z0, nzc, stream); }
  return hipErrorInvalidValue;
}
hipError_t launch_rebrick(const VolumeDesc& general, void* dst, const VolumeDesc& vd, hipStream_t stream)
{
  for (int z0 = 0; z0 < vd.nz; z0 += 32768) { // grid.z limit
    const int nzc = std::min(32768, vd.nz - z0);
    hipError_t e = hipErrorInvalidValue;
    dispatch_general_voxel_type(general.type, [&](auto vtb) { e = rebrick_b<decltype(vtb)::value>(general, dst, vd, z0, nzc, stream); });
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ------------------------------------------------------------------------------------------------------------------
// ovr_hip_update_volume: the box-restricted siblings of relayout_kernel / relayout_quad_kernel.  The ranges of macro rows,
// layers, macro blocks and bricks come from host/update_extent.hpp; a kernel applies the per-row predicate "holds a copy of a voxel in the box"
// ------------------------------------------------------------------------------------------------------------------
// the caller's box array: voxel (x, y, z) of the volume for x, y, z inside the box
template <typename TI> struct SrcBox {
  typedef TI value_type;
  static constexpr bool kBox = true;
  const TI* p; int x0, y0, z0, ex, ey;
  __device__ __forceinline__ TI get(size_t x, size_t y, unsigned z) const { return p[(x - (size_t)x0) + (size_t)ex * ((y - (size_t)y0) + (size_t)ey * (size_t)(z - (unsigned)z0))]; }
};
// the box in the layout's axes (a = pair axis, b = the other one), voxels [lo, hi), and where the launch's grid starts
struct UpdateRows { int alo, ahi, blo, bhi, zlo, zhi; int brick_lo, brick_hi, macro_lo, macros, row_lo, layer_lo; };

// Rows in storage order like relayout_kernel's: a workgroup owns the slab of one macro row and one z layer and sweeps the macro blocks that meet the
// box, so where the box spans whole macro rows every 128-byte line still leaves the workgroup complete.  From the box array (SrcBox: the general
// layout) a row wholly inside the box is one unaligned vector load and one row store, a row partly inside is read, patched and stored; from the
// general layout (SrcBricked: a replica) the whole row is rewritten - its other elements are current in the source.  Padding rows are never touched.
template <typename SRC, typename TO, int VT>
__global__ __launch_bounds__(256) void update_rows_kernel(const SRC src, TO* __restrict__ dst, int nx, int ny, unsigned int macro_y, unsigned long long macro_z, const UpdateRows u)
{
  typedef typename SRC::value_type TI;
  typedef RowSweep<VT> S;
  typedef Vox<VT> V;
  constexpr bool TR = V::kTransposed;
  constexpr unsigned SX = S::SX;
  const int na = TR ? ny : nx;
  const unsigned my = (unsigned)u.row_lo + blockIdx.x, layer = (unsigned)u.layer_lo + blockIdx.y;
  const unsigned long long slab = S::slab(my, layer, macro_y, macro_z);
  const unsigned total = (unsigned)u.macros * S::ROWS;
  for (unsigned g = threadIdx.x; g < total; g += 256u) {
    const typename S::Row r = S::decode(g, (unsigned)u.macro_lo, my, layer);
    const int b = (int)r.b, z = (int)r.z;
    const int br = (int)r.br;
    if (b < u.blo || b >= u.bhi || z < u.zlo || z >= u.zhi || br < u.brick_lo || br > u.brick_hi) continue;
    RowOut<TO, SX>* const row = S::row(dst, slab, r);
    const int v0 = br * V::cx - 1;
    RowOut<TO, SX> out;
    if constexpr (SRC::kBox) {
      static_assert(!TR, "the caller's array goes into the general layout");
      if (v0 >= u.alo && v0 + (int)SX <= u.ahi) {
        const RowIn<TI, SX> w = *reinterpret_cast<const RowIn<TI, SX>*>(&src.p[((size_t)v0 - (size_t)src.x0) + (size_t)src.ex * (((size_t)b - (size_t)src.y0) + (size_t)src.ey * (size_t)(z - src.z0))]);
#pragma unroll
        for (unsigned k = 0; k < SX; ++k) out.v[k] = Conv<TI, TO>::cv(w.v[k]);
      }
      else {
        out = *row;
#pragma unroll
        for (unsigned k = 0; k < SX; ++k) {
          const int as = min(max(v0 + (int)k, 0), na - 1);
          if (as >= u.alo && as < u.ahi) out.v[k] = Conv<TI, TO>::cv(src.get((size_t)as, (size_t)b, (unsigned)z));
        }
      }
    }
    else {
#pragma unroll
      for (unsigned k = 0; k < SX; ++k) {
        const size_t as = (size_t)min(max(v0 + (int)k, 0), na - 1);
        out.v[k] = Conv<TI, TO>::cv(TR ? src.get((size_t)b, as, (unsigned)z) : src.get(as, (size_t)b, (unsigned)z));
      }
    }
    *row = out;
  }
}

// the cells [u_lo, u_hi] x [v_lo, v_hi] x [zlo, zhi) of a quad replica (the box grown by one cell: cell (u, v) holds x in { u - 1, u }, y in { v - 1, v })
struct UpdateCells { int u_lo, u_hi, v_lo, v_hi, zlo, zhi; int macro_lo, macros, row_lo, layer_lo; };
template <typename SRC, int VT>
__global__ __launch_bounds__(256) void update_quad_kernel(const SRC src, typename Vox<VT>::T* __restrict__ dst, int nx, int ny, unsigned int macro_y, unsigned long long macro_z,
                                                         const UpdateCells c)
{
  typedef typename SRC::value_type TI;
  typedef QuadSweep<VT> S;
  typedef BrickMap<VT> M;
  typedef Vox<VT> V;
  typedef typename V::T TO;
  typedef typename V::Q Q;
  const unsigned my = (unsigned)c.row_lo + blockIdx.x, layer = (unsigned)c.layer_lo + blockIdx.y;
  const unsigned long long slab = S::slab(my, layer, macro_y, macro_z);
  const unsigned total = (unsigned)c.macros * S::CELLS;
  for (unsigned g = threadIdx.x; g < total; g += 256u) {
    const unsigned ml = g / S::CELLS, i = g - ml * S::CELLS, mx = (unsigned)c.macro_lo + ml;
    const unsigned j = i & (S::CB - 1u), brick = i / S::CB;
    const int u = (int)(mx * 32u + ((brick & (M::bx_ - 1u)) << V::lx) + (j & ((1u << V::lx) - 1u)));
    const int v = (int)(my * 32u + ((brick / M::bx_) << V::ly) + ((j >> V::lx) & ((1u << V::ly) - 1u)));
    const int z = (int)((layer << V::lz) + (j >> (V::lx + V::ly)));
    if (u < c.u_lo || u > c.u_hi || v < c.v_lo || v > c.v_hi || z < c.zlo || z >= c.zhi) continue;
    Q* const cell = reinterpret_cast<Q*>(dst + slab + (unsigned long long)mx * M::MV + (unsigned long long)i * 4u);
    const int x = max(u - 1, 0), y = max(v - 1, 0);
    const int x1 = min(u, nx - 1), y1 = min(v, ny - 1);
    Q q;
    q.x = Conv<TI, TO>::cv(src.get((size_t)x, (size_t)y, (unsigned)z)); q.y = Conv<TI, TO>::cv(src.get((size_t)x1, (size_t)y, (unsigned)z));
    q.z = Conv<TI, TO>::cv(src.get((size_t)x, (size_t)y1, (unsigned)z)); q.w = Conv<TI, TO>::cv(src.get((size_t)x1, (size_t)y1, (unsigned)z));
    *cell = q;
  }
}

template <int VT> static update::Geometry update_geometry()
{
  typedef Vox<VT> V;
  update::Geometry g{ V::cx, V::mbx, V::by, V::bz, V::kTransposed, V::kQuad, 0, 0, 0 };
  if constexpr (V::kQuad) { g.lx = V::lx; g.ly = V::ly; g.lz = V::lz; }
  return g;
}
constexpr int kUpdateLayers = 32768; // z layers per launch (grid.y)

template <typename SRC, typename TO, int VT>
static hipError_t update_rows_s(const SRC& src, void* dst, const VolumeDesc& vd, const update::Box& box, hipStream_t stream)
{
  const int dims[3] = { vd.nx, vd.ny, vd.nz };
  const update::BrickRange r = update::brick_range(update_geometry<VT>(), dims, vd.macros_x, box);
  constexpr int ia = Vox<VT>::kTransposed ? 1 : 0, ib = Vox<VT>::kTransposed ? 0 : 1;
  for (int l0 = r.layer_lo; l0 <= r.layer_hi; l0 += kUpdateLayers) {
    const UpdateRows u{ box.lo[ia], box.hi[ia], box.lo[ib], box.hi[ib], box.lo[2], box.hi[2], r.brick_lo, r.brick_hi, r.macro_lo, r.macro_hi - r.macro_lo + 1, r.row_lo, l0 };
    const dim3 grid((unsigned)(r.row_hi - r.row_lo + 1), (unsigned)(std::min(r.layer_hi, l0 + kUpdateLayers - 1) - l0 + 1));
    hipLaunchKernelGGL((update_rows_kernel<SRC, TO, VT>), grid, dim3(256), 0, stream, src, (TO*)dst, vd.nx, vd.ny, macro_stride_y(vd), macro_stride_z(vd), u);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}
template <typename SRC, int VT>
static hipError_t update_quad_s(const SRC& src, void* dst, const VolumeDesc& vd, const update::Box& box, hipStream_t stream)
{
  const update::QuadRange r = update::quad_range(update_geometry<VT>(), box);
  for (int l0 = r.layer_lo; l0 <= r.layer_hi; l0 += kUpdateLayers) {
    const UpdateCells c{ r.u_lo, r.u_hi, r.v_lo, r.v_hi, box.lo[2], box.hi[2], r.macro_lo, r.macro_hi - r.macro_lo + 1, r.row_lo, l0 };
    const dim3 grid((unsigned)(r.row_hi - r.row_lo + 1), (unsigned)(std::min(r.layer_hi, l0 + kUpdateLayers - 1) - l0 + 1));
    hipLaunchKernelGGL((update_quad_kernel<SRC, VT>), grid, dim3(256), 0, stream, src, (typename Vox<VT>::T*)dst, vd.nx, vd.ny, macro_stride_y(vd), macro_stride_z(vd), c);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}
hipError_t launch_update_general(const void* src, int vt, void* dst, const VolumeDesc& vd, const update::Box& box, hipStream_t stream)
{
  hipError_t e = hipErrorInvalidValue; // as launch_relayout: the same Conv per element
  dispatch_value_type(vt, [&](auto v) {
    typedef decltype(v) V;
    typedef SrcBox<typename V::TI> Src;
    if (vd.type == V::VT)
      e = update_rows_s<Src, typename V::TO, V::VT>(Src{ (const typename V::TI*)src, box.lo[0], box.lo[1], box.lo[2], box.hi[0] - box.lo[0], box.hi[1] - box.lo[1] }, dst, vd, box, stream);
  });
  return e;
}
template <int VTB>
static hipError_t update_replica_b(const VolumeDesc& g, void* dst, const VolumeDesc& vd, const update::Box& box, hipStream_t stream)
{
  typedef typename Vox<VTB>::T T;
  typedef SrcBricked<VTB> Src;
  constexpr int T1 = replica_voxel_type(VTB, LAYOUT_THIN), T2 = replica_voxel_type(VTB, LAYOUT_THIN_T), TQ = replica_voxel_type(VTB, LAYOUT_QUAD);
  if constexpr (TQ >= 0) { if (vd.type == TQ) return update_quad_s<Src, TQ>(src_bricked<VTB>(g), dst, vd, box, stream); }
  if constexpr (T1 >= 0) { if (vd.type == T1) return update_rows_s<Src, T, T1>(src_bricked<VTB>(g), dst, vd, box, stream); }
  if constexpr (T2 >= 0) { if (vd.type == T2) return update_rows_s<Src, T, T2>(src_bricked<VTB>(g), dst, vd, box, stream); }
  return hipErrorInvalidValue;
}
hipError_t launch_update_replica(const VolumeDesc& general, void* dst, const VolumeDesc& vd, const update::Box& box, hipStream_t stream)
{
  hipError_t e = hipErrorInvalidValue;
  dispatch_general_voxel_type(general.type, [&](auto vtb) { e = update_replica_b<decltype(vtb)::value>(general, dst, vd, box, stream); });
  return e;
}

// per-axis offset tables of a layout (VolumeDesc::axis_ab / axis_z), once per volume
template <int VT>
__global__ __launch_bounds__(256) void axis_tables_kernel(VolumeDesc vd, unsigned int* __restrict__ ab, unsigned long long* __restrict__ tz)
{
  typedef BrickMap<VT> M;
  const int na = Vox<VT>::kTransposed ? vd.ny : vd.nx, nb = Vox<VT>::kTransposed ? vd.nx : vd.ny;
  const unsigned int macro_y = macro_stride_y(vd);
  const unsigned long long macro_z = macro_stride_z(vd);
  // entry i of a table belongs to voxel index i - 1 (VolumeDesc): a = -1 ... na - 1 (lower member of the pair; stored position i),
  // b and z = -1 ... n with the indices clamped into the grid; a quad replica's cells are (x + 1, y + 1), its y entry i is cell i
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < axis_a_entries(na)) ab[i] = M::X((unsigned)i);
  if (i < axis_b_entries(nb)) ab[axis_a_entries(na) + i] = M::Y(Vox<VT>::kQuad ? (unsigned)min(i, nb) : (unsigned)min(max(i - 1, 0), nb - 1), macro_y);
  if (i < axis_z_entries(vd.nz)) {
    const unsigned z = (unsigned)min(max(i - 1, 0), vd.nz - 1);
    tz[i] = (unsigned long long)M::Zlo(z) + (unsigned long long)(z >> 5) * macro_z;
  }
}
size_t axis_table_bytes(const VolumeDesc& vd)
{
  return (size_t)axis_z_entries(vd.nz) * sizeof(unsigned long long) + (size_t)(vd.nx + vd.ny + 3) * sizeof(unsigned int);
}
template <int VT>
static hipError_t axis_tables_t(const VolumeDesc& vd, unsigned int* ab, unsigned long long* tz, hipStream_t stream)
{
  const int n = std::max(std::max(vd.nx, vd.ny), vd.nz) + 2;
  hipLaunchKernelGGL(axis_tables_kernel<VT>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, vd, ab, tz);
  return hipGetLastError();
}
hipError_t launch_axis_tables(VolumeDesc& vd, void* d_tables, hipStream_t stream)
{
  unsigned long long* tz = static_cast<unsigned long long*>(d_tables);
  unsigned int* ab = reinterpret_cast<unsigned int*>(tz + axis_z_entries(vd.nz));
  vd.axis_z = tz;
  vd.axis_ab = ab;
  hipError_t e = hipErrorInvalidValue;
  dispatch_voxel_type(vd.type, [&](auto vt) { e = axis_tables_t<decltype(vt)::value>(vd, ab, tz, stream); });
  return e;
}

// ------------------------------------------------------------------------------------------------------------------
// macrocells (reference ovr/devices/optix7/accel/sp_singlemc.cu): 16^3-voxel cells with a value range and, per transfer
// function, the largest opacity any sample inside can get.  The reference builds both grids but only its path tracer uses
// them; here the ray marcher and the shadow march skip the voxel fetch of samples whose cell has majorant 0 - such a
// sample's opacity is exactly 0, so frames are bit-identical with and without skipping.
// ------------------------------------------------------------------------------------------------------------------
// value_range_kernel, sp_singlemc.cu:10-54: one WAVE per macrocell (the reference uses one thread), wave min/max reduction.
// A lane owns (y, z) ROWS of the cell's 18^3 box - rows in storage order, so the four lanes of a quad read 64 contiguous bytes - and walks each
// along x brick by brick: one 8- or 16-byte load per brick row (SX stored voxels), the voxels outside the box masked.  (Until round 4: one voxel per
// lane and step, each with its own offset arithmetic and three runtime divisions - 2.8 ms for C3, 20.6 ms for C4, bound by the gather-instruction rate.)
// (the value range of cell (cx, cy, cz), reduced over the wave: what macrocell_range_kernel computes for every cell and macrocell_range_box_kernel for the
// cells an ovr_hip_update_volume touched - one text, so a recomputed cell is a full rebuild's bit for bit)
template <int VT>
__device__ __forceinline__ float2 macrocell_cell_range(const void* __restrict__ vol, const VolumeDesc& vd, int cx, int cy, int cz, int lane)
{
  typedef BrickMap<VT> M;
  typedef Vox<VT> V;
  typedef typename V::T T;
  constexpr unsigned SX = M::SX, HY = 1u << V::by, HZ = 1u << V::bz;   // a brick: SX x HY x HZ stored voxels
  constexpr int W = 16;
  // brick-aligned spans that hold W + 2 rows at any alignment
  constexpr unsigned AY = (W + 2 + 2 * (HY - 1) + HY - 1) / HY, AZ = (W + 2 + 2 * (HZ - 1) + HZ - 1) / HZ; // in bricks
  const int bx = max(cx * W - 1, 0), by = max(cy * W - 1, 0), bz = max(cz * W - 1, 0);
  const int ex = min(bx + W + 1, vd.nx), ey = min(by + W + 1, vd.ny), ez = min(bz + W + 1, vd.nz);
  const unsigned macro_y = macro_stride_y(vd);
  const unsigned long long macro_z = macro_stride_z(vd);
  const T* base = static_cast<const T*>(vol);
  // voxel x is stored at position x + 1: brick (x + 1) / cx, whose row holds the voxels brick * cx - 1 ... brick * cx + cx - 1
  const unsigned b0 = M::div_cx((unsigned)bx + 1u), nbx = M::div_cx((unsigned)ex) - b0 + 1u; // the bricks along x that hold voxels bx ... ex - 1
  const unsigned ya = (unsigned)by & ~(HY - 1u), za = (unsigned)bz & ~(HZ - 1u);
  float lo = INFINITY, hi = -INFINITY; // range1f() is empty
  for (unsigned t = (unsigned)lane; t < AY * AZ * HY * HZ; t += 64u) {
    const unsigned q = t / (HY * HZ);
    const unsigned y = ya + (q % AY) * HY + (t & (HY - 1u)), z = za + (q / AY) * HZ + ((t / HY) & (HZ - 1u));
    if ((int)y < by || (int)y >= ey || (int)z < bz || (int)z >= ez) continue;
    const unsigned long long row = (unsigned long long)M::Y(y, macro_y) + M::Zlo(z) + (unsigned long long)(z >> 5) * macro_z;
    for (unsigned qx = 0; qx < nbx; ++qx) {
      const unsigned br = b0 + qx;
      const unsigned m = M::div_mbx(br), bm = br - m * V::mbx;
      const RowOut<T, SX> w = *reinterpret_cast<const RowOut<T, SX>*>(base + (row + (bm * M::BV + m * M::MV)));
      const int v0 = (int)(br * V::cx) - 1; // the voxel of the row's first element
#pragma unroll
      for (unsigned k = 0; k < SX; ++k) {
        float f = (float)w.v[k];
        if (VT == VOX_U8) f = f / 255.f;                            // what the normalized texture read returns (array.cpp:304-306)
        if (VT == VOX_I8) { f = f / 127.f; f = f < -1.f ? -1.f : f; }
        const bool in = v0 + (int)k >= bx && v0 + (int)k < ex;
        lo = in ? fminf(lo, f) : lo;
        hi = in ? fmaxf(hi, f) : hi;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off));
    hi = fmaxf(hi, __shfl_xor(hi, off));
  }
  return make_float2(lo, hi);
}
template <int VT>
__global__ __launch_bounds__(256) void macrocell_range_kernel(const void* __restrict__ vol, VolumeDesc vd, int mcx, int mcy, int mcz, float2* __restrict__ out)
{
  const int lane = threadIdx.x & 63;
  const unsigned long long cell = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= (unsigned long long)mcx * mcy * mcz) return;
  const int cx = (int)(cell % mcx), cy = (int)((cell / mcx) % mcy), cz = (int)(cell / ((unsigned long long)mcx * mcy));
  const float2 r = macrocell_cell_range<VT>(vol, vd, cx, cy, cz, lane);
  if (lane == 0) out[cell] = r;
}
// ovr_hip_update_volume: the cells lo ... lo + n - 1 per axis alone
template <int VT>
__global__ __launch_bounds__(256) void macrocell_range_box_kernel(const void* __restrict__ vol, VolumeDesc vd, int mcx, int mcy, int lx, int ly, int lz, int nx, int ny, int nz,
                                                                 float2* __restrict__ out)
{
  const int lane = threadIdx.x & 63;
  const unsigned long long s = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= (unsigned long long)nx * ny * nz) return;
  const int cx = lx + (int)(s % nx), cy = ly + (int)((s / nx) % ny), cz = lz + (int)(s / ((unsigned long long)nx * ny));
  const float2 r = macrocell_cell_range<VT>(vol, vd, cx, cy, cz, lane);
  if (lane == 0) out[(unsigned long long)cx + (unsigned long long)mcx * ((unsigned long long)cy + (unsigned long long)mcy * (unsigned long long)cz)] = r;
}

// majorant_kernel, sp_singlemc.cu:56-97: the alpha table is staged in LDS exactly as the reference stages it in shared memory
__global__ __launch_bounds__(256) void macrocell_majorant_kernel(const float2* __restrict__ ranges, unsigned int count, const float* __restrict__ alphas, int n_alpha,
                                                                float vr_lo, float vr_hi, float* __restrict__ out)
{
  extern __shared__ float lds_alpha[];
  for (int i = threadIdx.x; i < n_alpha; i += 256) lds_alpha[i] = alphas[i];
  __syncthreads();
  const unsigned int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const float2 r = ranges[i];
  const float rcp = 1.f / (vr_hi - vr_lo);
  const float lower = (fminf(fmaxf(r.x, vr_lo), vr_hi) - vr_lo) * rcp;
  const float upper = (fminf(fmaxf(r.y, vr_lo), vr_hi) - vr_lo) * rcp;
  const float fl = floorf(fmaf(lower, (float)(n_alpha - 1), 0.5f)) - 1.f;
  const float fu = floorf(fmaf(upper, (float)(n_alpha - 1), 0.5f)) + 1.f;
  unsigned int il = fl < 0.f ? 0u : (unsigned int)fl; // float -> uint32 saturates in the reference's device code
  unsigned int iu = fu < 0.f ? 0u : (unsigned int)fu;
  il = min(il, (unsigned int)(n_alpha - 1));
  iu = min(iu, (unsigned int)(n_alpha - 1));
  float op = 0.f;
  for (unsigned int k = il; k <= iu; ++k) op = fmaxf(op, lds_alpha[k]);
  out[i] = op;
}

hipError_t launch_macrocell_ranges(const VolumeDesc& vd, float* out_minmax, hipStream_t stream)
{
  const int mcx = (vd.nx + 15) / 16, mcy = (vd.ny + 15) / 16, mcz = (vd.nz + 15) / 16;
  const unsigned long long cells = (unsigned long long)mcx * mcy * mcz;
  const dim3 grid((unsigned)((cells + 3) / 4)), block(256);
  if (!dispatch_general_voxel_type(vd.type, [&](auto vt) {
        hipLaunchKernelGGL(macrocell_range_kernel<decltype(vt)::value>, grid, block, 0, stream, vd.data, vd, mcx, mcy, mcz, (float2*)out_minmax);
      }))
    return hipErrorInvalidValue; // the macrocells are computed from the general layout
  return hipGetLastError();
}

hipError_t launch_macrocell_ranges_box(const VolumeDesc& vd, float* out_minmax, const update::CellRange& c, hipStream_t stream)
{
  const int mcx = (vd.nx + 15) / 16, mcy = (vd.ny + 15) / 16, mcz = (vd.nz + 15) / 16;
  const int nx = c.hi[0] - c.lo[0] + 1, ny = c.hi[1] - c.lo[1] + 1, nz = c.hi[2] - c.lo[2] + 1;
  if (c.lo[0] < 0 || c.lo[1] < 0 || c.lo[2] < 0 || nx < 1 || ny < 1 || nz < 1 || c.hi[0] >= mcx || c.hi[1] >= mcy || c.hi[2] >= mcz) return hipErrorInvalidValue;
  const unsigned long long cells = (unsigned long long)nx * ny * nz;
  const dim3 grid((unsigned)((cells + 3) / 4)), block(256);
  if (!dispatch_general_voxel_type(vd.type, [&](auto vt) {
        hipLaunchKernelGGL(macrocell_range_box_kernel<decltype(vt)::value>, grid, block, 0, stream, vd.data, vd, mcx, mcy, c.lo[0], c.lo[1], c.lo[2], nx, ny, nz, (float2*)out_minmax);
      }))
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_macrocell_majorants(const float* minmax, unsigned int count, const float* alphas, int n_alpha, float vr_lo, float vr_hi, float* out,
                                      hipStream_t stream)
{
  hipLaunchKernelGGL(macrocell_majorant_kernel, dim3((count + 255) / 256), dim3(256), (size_t)n_alpha * sizeof(float), stream, (const float2*)minmax, count, alphas,
                     n_alpha, vr_lo, vr_hi, out);
  return hipGetLastError();
}

// the volume's data range: min / max over all macrocell ranges (every voxel lies in at least one cell); fminf / fmaxf drop
// NaN operands like the reference's std::min / std::max chain does (array.cpp:44-62)
// two launches: kMinmaxBlocks workgroups reduce a slice each into out[2 + 2 b ...], one workgroup reduces those (one workgroup over all cells
// took 0.94 ms for C4's 2 M cells)
constexpr int kMinmaxBlocks = 256;
__global__ __launch_bounds__(256) void minmax_reduce_kernel(const float2* __restrict__ ranges, unsigned long long cells, float* __restrict__ out, int final_pass)
{
  __shared__ float slo[4], shi[4];
  float lo = FLT_MAX, hi = -FLT_MAX; // numeric_limits<float>::max() / lowest()
  const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < cells; i += stride) {
    const float2 r = ranges[i];
    lo = fminf(lo, r.x);
    hi = fmaxf(hi, r.y);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off));
    hi = fmaxf(hi, __shfl_xor(hi, off));
  }
  if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) { lo = fminf(lo, slo[w]); hi = fmaxf(hi, shi[w]); }
    float* o = final_pass ? out : out + 2 + 2 * blockIdx.x;
    o[0] = lo;
    o[1] = hi;
  }
}
size_t minmax_reduce_floats() { return 2 + 2 * (size_t)kMinmaxBlocks; }
hipError_t launch_minmax_reduce(const float* minmax, unsigned long long cells, float* out, hipStream_t stream)
{
  hipLaunchKernelGGL(minmax_reduce_kernel, dim3(kMinmaxBlocks), dim3(256), 0, stream, (const float2*)minmax, cells, out, 0);
  hipLaunchKernelGGL(minmax_reduce_kernel, dim3(1), dim3(256), 0, stream, (const float2*)(out + 2), (unsigned long long)kMinmaxBlocks, out, 1);
  return hipGetLastError();
}

// occupancy for the per-ray skip interval (skip_interval), two levels: a coarse grid of 4^3 macrocells (64^3 voxels) per entry -
// small enough (4 KiB at 1024^3) to stay in L1 while every ray walks it - and a fine grid of one entry per macrocell, walked only
// inside the coarse interval.  An entry is set if any of its macrocells, or any macrocell next to one of them (dilation by one
// macrocell), can hold a sample with opacity > 0.  The dilation is the safety margin of the walk: a ray's cell sequence is right
// to ~1e-4 voxel of position, the nearest non-empty sample is >= 16 voxels inside a set entry.   S = macrocells per entry and axis
__global__ __launch_bounds__(256) void macrocell_coarse_kernel(const float* __restrict__ majorant, int mcx, int mcy, int mcz, int S, unsigned char* __restrict__ out)
{
  const int gx = (mcx + S - 1) / S, gy = (mcy + S - 1) / S, gz = (mcz + S - 1) / S;
  const unsigned int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (unsigned int)(gx * gy * gz)) return;
  const int cx = (int)(i % (unsigned int)gx) * S, cy = (int)((i / (unsigned int)gx) % (unsigned int)gy) * S, cz = (int)(i / (unsigned int)(gx * gy)) * S;
  bool any = false;
  for (int z = max(cz - 1, 0); z <= min(cz + S, mcz - 1); ++z)
    for (int y = max(cy - 1, 0); y <= min(cy + S, mcy - 1); ++y)
      for (int x = max(cx - 1, 0); x <= min(cx + S, mcx - 1); ++x)
        any = any || (majorant[(size_t)x + (size_t)mcx * ((size_t)y + (size_t)mcy * (size_t)z)] > 0.f);
  out[i] = any ? 1 : 0;
}
// the coarse grid from the fine one: an entry's dilated 6^3 neighbourhood is the union of the dilated neighbourhoods of its 4^3
// macrocells, so it is the OR of 64 fine entries - one wave per coarse entry, one fine entry per lane (the direct form, one THREAD
// per coarse entry reading 216 majorants, took 0.4 ms at 1024^3: on every transfer-function edit)
__global__ __launch_bounds__(256) void macrocell_coarse_from_fine_kernel(const unsigned char* __restrict__ fine, int mcx, int mcy, int mcz, unsigned char* __restrict__ out)
{
  const int gx = (mcx + 3) / 4, gy = (mcy + 3) / 4, gz = (mcz + 3) / 4;
  const unsigned int i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= (unsigned int)(gx * gy * gz)) return; // wave-uniform
  const int lane = threadIdx.x & 63;
  const int x = (int)(i % (unsigned int)gx) * 4 + (lane & 3), y = (int)((i / (unsigned int)gx) % (unsigned int)gy) * 4 + ((lane >> 2) & 3),
            z = (int)(i / (unsigned int)(gx * gy)) * 4 + (lane >> 4);
  const bool set = x < mcx && y < mcy && z < mcz && fine[(size_t)x + (size_t)mcx * ((size_t)y + (size_t)mcy * (size_t)z)] != 0;
  const unsigned long long any = __ballot(set);
  if (lane == 0) out[i] = any != 0ull ? 1 : 0;
}
hipError_t launch_macrocell_coarse(const float* majorant, int nx, int ny, int nz, unsigned char* out_coarse, unsigned char* out_fine, hipStream_t stream)
{
  const int mcx = (nx + 15) / 16, mcy = (ny + 15) / 16, mcz = (nz + 15) / 16;
  const unsigned int coarse = (unsigned int)(((mcx + 3) / 4) * ((mcy + 3) / 4) * ((mcz + 3) / 4)), fine = (unsigned int)(mcx * mcy * mcz);
  hipLaunchKernelGGL(macrocell_coarse_kernel, dim3((fine + 255) / 256), dim3(256), 0, stream, majorant, mcx, mcy, mcz, 1, out_fine);
  hipLaunchKernelGGL(macrocell_coarse_from_fine_kernel, dim3((coarse + 3) / 4), dim3(256), 0, stream, out_fine, mcx, mcy, mcz, out_coarse);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// sparse-sampling mask: noise tile slice staged in LDS, keep test, wave64 ballot + prefix compaction
// (generate_mask.cu:55-96; the reference compacts with thrust::remove, which keeps pixel order - so does this)
// ------------------------------------------------------------------------------------------------------------------
// __expf restated as a fixed sequence of IEEE basic operations, so the integer keep/discard decision is reproducible
// bit for bit (2^n * 2^f with a degree-6 Horner polynomial; relative error 2e-7 near 0, 2e-6 at x = -30: inside __expf's own bound of 2 + |1.16 x| ulp)
__device__ __forceinline__ float exp_det(float x)
{
  if (x < -87.f) return 0.f;
  if (x > 88.f) x = 88.f;
  const float t = x * 1.44269504088896341f;
  const float n = floorf(t + 0.5f);
  const float f = t - n;
  float p = 1.53533031e-4f;
  p = fmaf(p, f, 1.33988696e-3f);
  p = fmaf(p, f, 9.61843120e-3f);
  p = fmaf(p, f, 5.55033022e-2f);
  p = fmaf(p, f, 2.40226504e-1f);
  p = fmaf(p, f, 6.93147182e-1f);
  p = fmaf(p, f, 1.0f);
  return p * __uint_as_float((unsigned int)((int)n + 127) << 23);
}

// The noise tile is stored transposed, [t][y][x] (the reference's file is [y][x][t], blue_noise.h:95-99), so the slice of one
// frame is a contiguous xy x xy block (16 - 64 KiB) instead of one float every 256 bytes.  A workgroup covers 256 consecutive
// pixels = at most two image rows; the noise rows they need are staged in LDS (lds_noise[2][xy]) with coalesced loads.
__device__ __forceinline__ void stage_noise_rows(const SparseMaskParams& p, float* lds_noise, unsigned int first_pixel)
{
  const int xy = p.noise_xy;
  const float* slice = p.noise + (size_t)(p.frame_index % 64) * xy * xy;
  const int y0 = (int)(first_pixel / (unsigned int)p.width);
  for (int i = threadIdx.x; i < 2 * xy; i += 256) {
    const int r = i / xy, c = i - r * xy;
    lds_noise[i] = slice[(size_t)((y0 + r) % xy) * xy + c];
  }
  __syncthreads();
}

// enumeration index -> pixel.  Row-major: i = x + y * W.  Tile-major (p.tile_major): 256 consecutive indices are one 16x16-pixel tile in
// Morton order (16 consecutive indices are a 4x4 block, 64 an 8x8 block); pixels beyond the image edge are never kept
__device__ __forceinline__ bool mask_pixel(const SparseMaskParams& p, unsigned int i, int& x, int& y)
{
  if (!p.tile_major) {
    x = (int)(i % (unsigned int)p.width);
    y = (int)(i / (unsigned int)p.width);
    return i < (unsigned int)p.width * (unsigned int)p.height;
  }
  const unsigned int tiles_x = ((unsigned int)p.width + 15u) / 16u;
  const unsigned int tile = i >> 8, in = i & 255u;
  // Morton (Z) order inside the tile: wherever the mask keeps only part of the pixels, 16 consecutive KEPT pixels - a wave's rays - are
  // still a compact patch (a 4x4 block where everything is kept, ~7x7 pixels at 30 %) instead of a 4-pixel-high strip of sub-tiles;
  // rays that are neighbours share bricks, and the sparse frame is bound by the lines its rays do not share (profiles/r03_notes.md)
  const unsigned int lx = (in & 1u) | ((in >> 1) & 2u) | ((in >> 2) & 4u) | ((in >> 3) & 8u);
  const unsigned int ly = ((in >> 1) & 1u) | ((in >> 2) & 2u) | ((in >> 3) & 4u) | ((in >> 4) & 8u);
  x =(int)((tile % tiles_x) * 16u + lx);
  y = (int)((tile / tiles_x) * 16u + ly);
  return x < p.width && y < p.height;
}

__device__ __forceinline__ bool mask_keep(const SparseMaskParams& p, const float* lds_noise, unsigned int first_pixel, unsigned int i, int& x, int& y)
{
  if (!mask_pixel(p, i, x, y)) return false;
  const int xy = p.noise_xy;
  float val;
  if (p.tile_major) val = p.noise[(size_t)(p.frame_index % 64) * xy * xy + (size_t)(y % xy) * xy + (x % xy)]; // a 16x16 patch of the slice: cached
  else {
    const int r = y - (int)(first_pixel / (unsigned int)p.width); // 0 or 1 (a third row only if width < 128: read the slice directly)
    val = r < 2 ? lds_noise[r * xy + (x % xy)] : p.noise[(size_t)(p.frame_index % 64) * xy * xy + (size_t)(y % xy) * xy + (x % xy)];
  }
  const float aspect = (float)p.width / p.height;
  const float fx = ((float)x / p.width - p.mean_x);
  const float fy = ((float)y / p.height - p.mean_y) / aspect;
  const float pr = (1.0f - p.base_noise) * exp_det(-0.5f * (fx * fx + fy * fy) * p.sigma_rcp2) + p.base_noise;
  return val < pr;
}

__global__ __launch_bounds__(256) void mask_count_kernel(const SparseMaskParams p)
{
  __shared__ unsigned int wave_cnt[4];
  __shared__ float lds_noise[2 * 128];
  const unsigned int i = blockIdx.x * 256 + threadIdx.x;
  if (!p.tile_major) stage_noise_rows(p, lds_noise, blockIdx.x * 256);
  int x, y;
  const bool keep = mask_keep(p, lds_noise, blockIdx.x * 256, i, x, y);
  const unsigned long long b = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = (unsigned int)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) p.block_counts[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// exclusive scan of block_counts in place (single workgroup, serial over chunks of 1024)
__global__ __launch_bounds__(1024) void mask_scan_kernel(unsigned int* counts, int n_blocks, unsigned long long* total)
{
  __shared__ unsigned int wsum[16];
  __shared__ unsigned int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int base = 0; base < n_blocks; base += 1024) {
    const int i = base + threadIdx.x;
    const unsigned int v = (i < n_blocks) ? counts[i] : 0u;
    unsigned int s = v; // inclusive scan within the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned int t = __shfl_up(s, off);
      if (lane >= off) s += t;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    unsigned int wbase = 0;
    for (int w = 0; w < wave; ++w) wbase += wsum[w];
    const unsigned int c = carry;
    if (i < n_blocks) counts[i] = c + wbase + s - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = c + wbase + s;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = 2ull * carry;
}

__global__ __launch_bounds__(256) void mask_write_kernel(const SparseMaskParams p)
{
  __shared__ unsigned int wave_cnt[4];
  __shared__ float lds_noise[2 * 128];
  const unsigned int i = blockIdx.x * 256 + threadIdx.x;
  if (!p.tile_major) stage_noise_rows(p, lds_noise, blockIdx.x * 256);
  int x = 0, y = 0;
  const bool keep = mask_keep(p, lds_noise, blockIdx.x * 256, i, x, y);
  const unsigned long long b = __ballot(keep);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // prefix of the ballot below this lane = v_mbcnt
  const unsigned int prefix = __builtin_amdgcn_mbcnt_hi((unsigned int)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)b, 0u));
  if (lane == 0) wave_cnt[wave] = (unsigned int)__popcll(b);
  __syncthreads();
  unsigned int off = p.block_counts[blockIdx.x];
  for (int w = 0; w < wave; ++w) off += wave_cnt[w];
  if (keep) {
    const size_t o = 2 * ((size_t)off + prefix);
    p.out_xy[o] = x;
    p.out_xy[o + 1] = y;
  }
}

static int mask_blocks(const SparseMaskParams& p)
{
  if (p.tile_major) return ((p.width + 15) / 16) * ((p.height + 15) / 16);
  return (int)(((size_t)p.width * p.height + 255) / 256);
}
// per-block counts of either enumeration order (+ 1): the tile-major order has at least as many blocks as the row-major one
size_t sparse_mask_workspace_elems(int width, int height) { return (size_t)((width + 15) / 16) * ((height + 15) / 16) + ((size_t)width * height + 255) / 256 + 1; }

hipError_t launch_sparse_mask(const SparseMaskParams& p, hipStream_t stream)
{
  const int n_blocks = mask_blocks(p);
  hipLaunchKernelGGL(mask_count_kernel, dim3(n_blocks), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(mask_scan_kernel, dim3(1), dim3(1024), 0, stream, p.block_counts, n_blocks, p.count);
  hipLaunchKernelGGL(mask_write_kernel, dim3(n_blocks), dim3(256), 0, stream, p);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// TEA known-answer entry
// ------------------------------------------------------------------------------------------------------------------
__global__ void tea_kernel(uint32_t* v0v1, float* out, long long n)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned int v0 = v0v1[2 * i], v1 = v0v1[2 * i + 1];
  tea16(v0, v1);
  v0v1[2 * i] = v0; v0v1[2 * i + 1] = v1;
  out[2 * i] = (float)v0 * OVR_TEA_TOFLOAT;
  out[2 * i + 1] = (float)v1 * OVR_TEA_TOFLOAT;
}
hipError_t launch_tea(uint32_t* v0v1, float* out, int64_t n, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(tea_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, v0v1, out, (long long)n);
  return hipGetLastError();
}

// known-answer entry of the pow the kernels evaluate for __powf (shaders_raymarching.cu:64-66,118-122): which = 0 the one this library was BUILT with
// (v_exp_f32(y * v_log_f32(x)), or the deterministic pair under -DOVR_PARITY_EXACT=1), 1 = the deterministic pair whatever the build
__global__ void pow_kernel(const float* x, const float* y, float* out, long long n, int which)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float xv = x[i], yv = y[i];
  out[i] = (which == 1 || OVR_PARITY_EXACT) ? det_powf(xv, yv) : __builtin_amdgcn_exp2f(yv * __builtin_amdgcn_logf(xv));
}
hipError_t launch_pow(const float* x, const float* y, float* out, int64_t n, int which, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(pow_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, y, out, (long long)n, which);
  return hipGetLastError();
}
int built_for_exact_parity() { return OVR_PARITY_EXACT; }

// known-answer entry of the shade factor: shade_light + shade_factor exactly as shade_request calls them, with the frame's parameter block
template <bool MAT, bool ORTHO = false>
__global__ void shade_floats_kernel(const RayMarchParams P, const float* normal_w, const float* pos, const float* shadow, float* out, long long n)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f3 n_w = mk3(normal_w[3 * i], normal_w[3 * i + 1], normal_w[3 * i + 2]), p = mk3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
  out[i] = shade_factor<MAT>(P, shade_light<MAT, ORTHO>(P, ld3(P.light), n_w, p), shadow[i]);
}
hipError_t launch_shade_floats(const RayMarchParams& p, const float* normal_w, const float* pos, const float* shadow, float* out, int64_t n, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  // as plan_launch picks the frame's kernels: an orthographic frame shades on the material variant (with the view vector -cam_dir)
  auto kern = p.cam_orthographic ? shade_floats_kernel<true, true> : reference_material(p) ? shade_floats_kernel<false> : shade_floats_kernel<true>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, normal_w, pos, shadow, out, (long long)n);
  return hipGetLastError();
}

// a frame's parameters as those of a known-answer query (or of the shadow cache's build): the frame's own machinery - request pool, majorants, sample list, block
// list, LDS staging - is not the query's; the macrocells' value ranges stay bound only where the query skips by them
static RayMarchParams query_params(const RayMarchParams& p, bool keep_ranges)
{
  RayMarchParams q = p;
  q.pool = PoolDesc{}; q.majorant = nullptr; q.sparse_xy = nullptr; q.schedule = nullptr; q.n_schedule = 0; q.lds_staging = 0;
  q.slice_context = 0;
  q.iso_context = 0; // (the context's own query puts it back)
  q.preintegrated = 0; // (likewise)
  q.gradient_opacity = 0; // (likewise)
  q.max_depth = nullptr; // (likewise)
  q.depth_tau = 0.f; // (likewise)
  q.slice_n = 0; // (committed slices take precedence in a FRAME's plan: the slices' own query puts them back)
  if (!keep_ranges) q.mc_ranges = nullptr;
  return q;
}
// the grid of a query kernel with four lanes per ray (n > 0); 0: more workgroups than a grid holds
static unsigned int quad_ray_blocks(int64_t n)
{
  const long long blocks = ((long long)n * 4 + kBlock - 1) / kBlock;
  return blocks > 0x7fffffffll ? 0u : (unsigned int)blocks;
}

// the shadow cache's build and the shadow march's known-answer entry (ShadowBuildArgs): the kernel of the general layout's type at the addressing mode the
// frame's kernels take for that layout (plan_launch: the layout's mode, the environment's override, the row loads)
hipError_t launch_shadow_cache(const RayMarchParams& p, const ShadowBuildArgs& a, hipStream_t stream)
{
  if (a.n <= 0) return hipSuccess;
  if (!a.out && !(a.pos_out && !a.pos)) return hipErrorInvalidValue; // nothing to write: out, or the nodes' positions alone
  RayMarchParams q = query_params(p, true);
  q.shading = 0; q.shadow_lattice = nullptr;
  q.iso_n = 0; q.ao_samples = 0; // (p may be a frame's parameters: the plan asked here is the march's, whatever the last frame drew)
  const LaunchPlan pl = plan_raymarch(q);
  if (pl.error) return hipErrorInvalidValue;
  ShadowCacheKernel kern = nullptr;
  dispatch_voxel_type(q.vol.type, [&](auto vt) { kern = shadow_cache_kernel_of<decltype(vt)::value>(pl.am); });
  if (!kern) return hipErrorInvalidValue;
  const size_t lds = align16(axis_table_bytes(q.vol.nx, q.vol.ny, q.vol.nz, pl.am)) + (size_t)q.n_alpha * 4 + 64;
  long long blocks;
  if (a.pos) blocks = (a.n + kBlock - 1) / kBlock;
  else {
    if (a.nx < 2 || a.ny < 2 || a.nz < 2 || (long long)a.nx * a.ny * a.nz != a.n) return hipErrorInvalidValue;
    const long long tiles = (long long)((a.nx + 3) / 4) * ((a.ny + 3) / 4) * ((a.nz + 3) / 4);
    blocks = (tiles + kWaves - 1) / kWaves;
  }
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
  return launch_variant(kern, dim3((unsigned)blocks), kBlock, lds, stream, q, a);
}

// known-answer entry of the lattice lookup: to_object as shade_request forms po, then shadow_lookup exactly as the cached kernels call it
__global__ void shadow_lookup_kernel(const RayMarchParams P, const float* pos, float* out, long long n)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  VolConsts vc;
  MarchConsts mc;
  setup_consts(P, vc, mc);
  out[i] = shadow_lookup(P, to_object(mc, mk3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2])));
}
hipError_t launch_shadow_lookup(const RayMarchParams& p, const float* pos, float* out, int64_t n, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  if (!p.shadow_lattice) return hipErrorInvalidValue;
  hipLaunchKernelGGL(shadow_lookup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, pos, out, (long long)n);
  return hipGetLastError();
}

// the known-answer ray queries (host/ray_query.hpp): the twin of the frame kernel of the query's kind, of the general layout's type at the addressing mode such a
// frame takes for it.  What the query does not ask about is scrubbed from the plan's facts, whatever is committed and whatever the last frame drew
hipError_t launch_ray_query(int query, const RayMarchParams& p, const RayQueryCall& c, hipStream_t stream)
{
  if (query < 0 || query >= kRayQueryTotal) return hipErrorInvalidValue;
  const RayQuery& d = ray_query_row(query);
  if (c.n <= 0) return hipSuccess;
  const bool skip = d.takes_range_skipping && c.range_skipping != 0 && !(d.takes_mode && c.mode == kProjectMean); // (a mean needs every sample: it has no skipping twin)
  if (skip && !p.mc_ranges) return hipErrorInvalidValue;
  if (d.needs == QueryNeeds::Slices && (p.slice_n < 1 || p.slice_n > kMaxSlices)) return hipErrorInvalidValue;
  if (d.needs == QueryNeeds::Isovalues && (p.iso_n < 1 || p.iso_n > kMaxIsovalues)) return hipErrorInvalidValue;
  if (d.takes_max_events && (c.max_events < 1 || c.max_events > kQueryMaxEvents)) return hipErrorInvalidValue;
  if (d.takes_rotation && (c.rotation < 0 || c.rotation >= kAoRotations)) return hipErrorInvalidValue;
  if (d.needs_ao && (p.ao_samples < 1 || p.ao_samples > kAoMaxSamples || !p.ao_dirs)) return hipErrorInvalidValue;
  if (d.needs_tf && (!p.tf_color || !p.tf_alpha)) return hipErrorInvalidValue;
  if (d.needs_preintegration && (!p.preint_nodes || p.preint_m1 < 1)) return hipErrorInvalidValue;
  if (d.takes_shade && (c.mode < 0 || c.mode > 1)) return hipErrorInvalidValue;
  if (d.takes_depth && !d.depth_optional && !c.depth) return hipErrorInvalidValue;
  if (d.takes_threshold && depth_output_check(kDepthOutputOn, c.threshold) != kDepthOutputOk) return hipErrorInvalidValue;
  RayMarchParams q = query_params(p, skip);
  switch (d.kind) {
  case FrameKind::Projection: q.projection = c.mode; q.iso_n = 0; q.ao_samples = 0; break; // (p may be an isosurface frame's parameters: the plan asked here is the projection's)
  case FrameKind::SliceWalk: q.slice_n = p.slice_n; break;
  case FrameKind::SliceContext: q.slice_n = p.slice_n; q.slice_context = 1; break;
  case FrameKind::Isosurface: q.iso_translucent = 0; q.ao_samples = 0; break;       // (the first crossing, opaque, whatever opacities and AO samples are committed)
  case FrameKind::IsosurfaceLayers: q.iso_translucent = 1; q.ao_samples = 0; break; // (without ambient occlusion, whatever is committed)
  case FrameKind::IsosurfaceContext: q.iso_context = 1; q.shading = 2; q.ao_samples = 0; break; // (under full shading)
  case FrameKind::IsosurfaceAo: q.iso_translucent = 1; q.shading = 2; break;        // (with full shading, the committed samples)
  case FrameKind::PreintegratedMarch: q.preintegrated = 1; q.shading = 0; q.projection = 0; q.iso_n = 0; q.ao_samples = 0; break; // (the unshaded march's plan, whatever is committed)
  case FrameKind::GradientOpacityMarch: q.gradient_opacity = 1; q.shading = c.mode; q.projection = 0; q.iso_n = 0; q.ao_samples = 0; break; // (the march's plan under the asked shading, whatever is committed)
  case FrameKind::DepthLimitedMarch: // (the march's plan under the asked shading, whatever is committed; the twin reads c.depth, one value per ray, never q.max_depth)
    q.max_depth = c.depth; q.shading = c.mode; q.projection = 0; q.iso_n = 0; q.ao_samples = 0;
    break;
  case FrameKind::DepthOutputMarch: // (likewise; c.depth may be null: no limit on any ray.  The plan reads depth_tau, the twin c.depth)
    q.depth_tau = c.threshold; q.max_depth = c.depth; q.shading = c.mode; q.projection = 0; q.iso_n = 0; q.ao_samples = 0;
    break;
  default: return hipErrorInvalidValue;
  }
  const LaunchPlan pl = plan_raymarch(q);
  if (pl.error || !query_runs(d, frame_kind(pl))) return hipErrorInvalidValue; // (the kernels are filed by signature: a plan of another kind must not lend its own)
  const PlanKernels k = plan_kernels(q, pl);
  const dim3 grid(quad_ray_blocks(c.n));
  if (d.takes_depth) return grid.x && k.query_depth ? launch_variant(k.query_depth, grid, kBlock, pl.march_lds_bytes, stream, q, c.org, c.dir, c.depth, c.out, c.n) : hipErrorInvalidValue;
  if (!grid.x || !(d.takes_rotation ? k.query_rotation != nullptr : d.takes_max_events ? k.query_events != nullptr : k.query != nullptr)) return hipErrorInvalidValue;
  if (d.zeroed)
    if (hipError_t e = hipMemsetAsync(c.out, 0, (size_t)c.n * ray_query_record_floats(d, c.max_events) * sizeof(float), stream)) return e;
  if (d.takes_rotation) return launch_variant(k.query_rotation, grid, kBlock, pl.march_lds_bytes, stream, q, c.org, c.dir, c.out, c.n, c.max_events, c.rotation);
  if (d.takes_max_events) return launch_variant(k.query_events, grid, kBlock, pl.march_lds_bytes, stream, q, c.org, c.dir, c.out, c.n, c.max_events);
  return launch_variant(k.query, grid, kBlock, pl.march_lds_bytes, stream, q, c.org, c.dir, c.out, c.n);
}

// known-answer entry of the box test: the object-space ray as the march forms it (to_object of the origin, the direction scaled by inv_scale, not
// renormalised), then box_test exactly as the march, the shadow march and the schedule call it
template <bool CLIP>
__global__ void clip_intervals_kernel(const RayMarchParams P, const float* org, const float* dir, float* out, long long n)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  VolConsts vc;
  MarchConsts mc;
  setup_consts(P, vc, mc);
  const f3 oo = to_object(mc, mk3(org[3 * i], org[3 * i + 1], org[3 * i + 2]));
  const f3 od = mk3(dir[3 * i] * mc.inv_scale.x, dir[3 * i + 1] * mc.inv_scale.y, dir[3 * i + 2] * mc.inv_scale.z);
  float t0 = 0.f, t1 = FLT_MAX;
  const bool hit = box_test<CLIP>(P, t0, t1, oo, od);
  out[3 * i] = t0; out[3 * i + 1] = t1; out[3 * i + 2] = hit ? 1.f : 0.f;
}
hipError_t launch_clip_intervals(const RayMarchParams& p, const float* org, const float* dir, float* t0t1hit, int64_t n, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  auto kern = p.clip_on ? clip_intervals_kernel<true> : clip_intervals_kernel<false>; // as plan_launch picks the frame's kernels
  hipLaunchKernelGGL(kern, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, org, dir, t0t1hit, (long long)n);
  return hipGetLastError();
}

// known-answer entry of the pixel ray: one lane per pixel; the screen position, the jitter of the sample and pixel_ray as the frame kernels form and call them
// (raymarch_kernel's in-place form: RandomTEA(frame_index, pixel_index) advanced once per sample when spp > 1, the blue-noise variates of jitter_global)
template <bool ORTHO>
__global__ __launch_bounds__(256) void camera_rays_kernel(const RayMarchParams P, int sample, float* __restrict__ out)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)P.width * P.height) return;
  const int ix = (int)(i % P.width), iy = (int)(i / P.width);
  const float rsx = 1.f / (float)P.width, rsy = 1.f / (float)P.height;
  float sx = ((float)ix + .5f) * rsx, sy = ((float)iy + .5f) * rsy;
  if (P.jitter_mode == 1) {
    float j0, j1;
    jitter_global(P, ix, iy, sample, j0, j1);
    sx += (j0 - 0.5f) * rsx;
    sy += (j1 - 0.5f) * rsy;
  }
  else if (P.spp > 1) {
    unsigned int v0 = (unsigned int)P.frame_index, v1 = (unsigned int)i;
    for (int k = 0; k <= sample; ++k) tea16(v0, v1);
    sx += ((float)v0 * OVR_TEA_TOFLOAT - 0.5f) * rsx;
    sy += ((float)v1 * OVR_TEA_TOFLOAT - 0.5f) * rsy;
  }
  const float ux = sx - 0.5f, uy = sy - 0.5f;
  f3 org, dir;
  pixel_ray<ORTHO>(P, ux, uy, org, dir);
  float* q = out + 6 * i;
  q[0] = org.x; q[1] = org.y; q[2] = org.z; q[3] = dir.x; q[4] = dir.y; q[5] = dir.z;
}
hipError_t launch_camera_rays(const RayMarchParams& p, int sample, float* org_dir, hipStream_t stream)
{
  const long long n = (long long)p.width * p.height;
  if (n <= 0) return hipSuccess;
  auto kern = p.cam_orthographic ? camera_rays_kernel<true> : camera_rays_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, sample, org_dir);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// tile pack / unpack (payload of the per-frame RCCL gather): slot k = k-th tile owned by `rank` in row-major tile order
// ------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int owned_in_row(int tiles_x, int ty, int rank, int world)
{
  const int first = ((rank - ty) % world + world) % world; // smallest tx with (tx + ty) % world == rank
  return first < tiles_x ? (tiles_x - 1 - first) / world + 1 : 0;
}
int count_owned_tiles(int width, int height, int tw, int th, int rank, int world)
{
  const int tiles_x = (width + tw - 1) / tw, tiles_y = (height + th - 1) / th;
  int n = 0;
  for (int ty = 0; ty < tiles_y; ++ty) n += owned_in_row(tiles_x, ty, rank, world);
  return n;
}

// slot of tile (tx, ty) in its owner's payload.  `world` consecutive tile rows hold every column exactly once per rank, so
// a rank owns tiles_x tiles per full period of rows; only the rows of the last, partial period are summed
__host__ __device__ inline int tile_slot(int tiles_x, int tx, int ty, int rank, int world)
{
  int slot = (ty / world) * tiles_x;
  for (int r = ty - ty % world; r < ty; ++r) slot += owned_in_row(tiles_x, r, rank, world);
  const int first = ((rank - ty) % world + world) % world;
  return slot + (tx - first) / world;
}

// one thread per frame pixel.  PACK: frame -> this rank's payload (pixels of foreign tiles exit).  !PACK: payload -> frame;
// rank >= 0 scatters that rank's payload, rank < 0 scatters ALL ranks' payloads, laid out `rank_stride` pixels apart, except
// `skip_rank`'s (the in-process device group: the gathering device rendered its own tiles in place).  C = floats per pixel: 4 = the
// RGBA layer, 3 = the gradient layer (device_impl.cpp:271-281 maps both)
template <bool PACK, int C>
__global__ __launch_bounds__(256) void tiles_kernel(const float* __restrict__ src, float* __restrict__ dst, int width, int height,
                                                   int tw, int th, int rank, int world, size_t rank_stride, int skip_rank)
{
  const int ix = blockIdx.x * 64 + (threadIdx.x & 63), iy = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (ix >= width || iy >= height) return;
  const int tx = ix / tw, ty = iy / th;
  const int owner = (tx + ty) % world;
  if (rank >= 0 ? owner != rank : owner == skip_rank) return;
  const int tiles_x = (width + tw - 1) / tw;
  const int slot = tile_slot(tiles_x, tx, ty, owner, world);
  const size_t pi = (size_t)slot * tw * th + (size_t)(iy - ty * th) * tw + (size_t)(ix - tx * tw) + (rank < 0 ? (size_t)owner * rank_stride : 0);
  const size_t fi = (size_t)iy * width + ix;
  const size_t si = PACK ? fi : pi, di = PACK ? pi : fi;
  if (C == 4) reinterpret_cast<float4*>(dst)[di] = reinterpret_cast<const float4*>(src)[si];
  else {
#pragma unroll
    for (int c = 0; c < C; ++c) dst[di * C + c] = src[si * C + c];
  }
}

hipError_t launch_pack_tiles(const float* frame, float* dst, int width, int height, int tw, int th, int rank, int world, hipStream_t stream, int channels)
{
  dim3 grid((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4));
  if (channels == 3) hipLaunchKernelGGL((tiles_kernel<true, 3>), grid, dim3(256), 0, stream, frame, dst, width, height, tw, th, rank, world, (size_t)0, -1);
  else hipLaunchKernelGGL((tiles_kernel<true, 4>), grid, dim3(256), 0, stream, frame, dst, width, height, tw, th, rank, world, (size_t)0, -1);
  return hipGetLastError();
}
hipError_t launch_unpack_tiles(const float* src, float* frame, int width, int height, int tw, int th, int rank, int world, size_t rank_stride_floats,
                               hipStream_t stream, int channels, int skip_rank)
{
  dim3 grid((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4));
  if (channels == 3) hipLaunchKernelGGL((tiles_kernel<false, 3>), grid, dim3(256), 0, stream, src, frame, width, height, tw, th, rank, world, rank_stride_floats / 3, skip_rank);
  else hipLaunchKernelGGL((tiles_kernel<false, 4>), grid, dim3(256), 0, stream, src, frame, width, height, tw, th, rank, world, rank_stride_floats / 4, skip_rank);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// frame output: image_to_rgba8 of the reference (ovr/common/imageio.cpp:146-181, 4 channels), on the device so that the
// host copy of a displayed / saved frame is 4 bytes per pixel instead of 16
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rgba8_kernel(const float4* __restrict__ rgba, uint32_t* __restrict__ out, int width, int height, int flip)
{
  const int ix = blockIdx.x * 64 + (threadIdx.x & 63), iy = blockIdx.y * 4 + (threadIdx.x >> 6); // output position
  if (ix >= width || iy >= height) return;
  const int sy = flip ? height - 1 - iy : iy;
  const float4 v = rgba[(size_t)sy * width + ix];
  // std::clamp(v, 0.f, 1.f) * 255.f, truncated (a NaN, undefined in the reference's cast, becomes 0)
  auto q = [](float x) -> uint32_t { return (uint32_t)(((x < 0.f) ? 0.f : (1.f < x) ? 1.f : x) * 255.f); };
  out[(size_t)iy * width + ix] = q(v.x) | (q(v.y) << 8) | (q(v.z) << 16) | (q(v.w) << 24);
}
hipError_t launch_rgba8(const float* rgba, uint32_t* out, int width, int height, int flip, hipStream_t stream)
{
  if (width <= 0 || height <= 0) return hipSuccess;
  dim3 grid((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4));
  hipLaunchKernelGGL(rgba8_kernel, grid, dim3(256), 0, stream, (const float4*)rgba, out, width, height, flip);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// frame output, EXR: the reference's save_image(".exr") hands the flipped RGBA32F frame to tinyexr and asks for HALF pixels
// (ovr/common/imageio.cpp:15-83,268-272).  The conversion on the device follows tinyexr's rule, which is NOT the hardware's
// v_cvt_f16_f32 (round to nearest even): the float mantissa is cut to 10 bits and its bit 12 rounds up (ties away from
// zero), the carry may run into the exponent; results below the half normal range shift the significand incl. the hidden
// bit and round by the last bit shifted out; float denormals -> signed 0, NaN -> quiet NaN 0x200, overflow -> infinity.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int exr_half_bits(float f)
{
  const unsigned int u = __float_as_uint(f);
  const unsigned int sign = (u >> 16) & 0x8000u, e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
  unsigned int h = 0u;
  if (e == 255u) h = 0x7c00u | (m ? 0x200u : 0u);
  else if (e != 0u) {
    const int ne = (int)e - 112; // re-biased exponent
    if (ne >= 31) h = 0x7c00u;
    else if (ne > 0) h = (((unsigned int)ne << 10) | (m >> 13)) + ((m >> 12) & 1u);
    else if (ne >= -10) {
      const unsigned int sig = m | 0x800000u;
      h = (sig >> (14 - ne)) + ((sig >> (13 - ne)) & 1u);
    }
  }
  return sign | h;
}
__global__ __launch_bounds__(256) void rgba16f_kernel(const float4* __restrict__ rgba, uint2* __restrict__ out, int width, int height, int flip)
{
  const int ix = blockIdx.x * 64 + (threadIdx.x & 63), iy = blockIdx.y * 4 + (threadIdx.x >> 6); // output position
  if (ix >= width || iy >= height) return;
  const int sy = flip ? height - 1 - iy : iy;
  const float4 v = rgba[(size_t)sy * width + ix];
  out[(size_t)iy * width + ix] = make_uint2(exr_half_bits(v.x) | (exr_half_bits(v.y) << 16), exr_half_bits(v.z) | (exr_half_bits(v.w) << 16));
}
hipError_t launch_rgba16f(const float* rgba, uint16_t* out, int width, int height, int flip, hipStream_t stream)
{
  if (width <= 0 || height <= 0) return hipSuccess;
  dim3 grid((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4));
  hipLaunchKernelGGL(rgba16f_kernel, grid, dim3(256), 0, stream, (const float4*)rgba, (uint2*)out, width, height, flip);
  return hipGetLastError();
}

} // namespace ovrhip
