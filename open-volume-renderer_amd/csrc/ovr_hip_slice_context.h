// ovr_hip_slice_context.h - the slice context (include/ovr_hip.h ovr_hip_set_slice_context; open-volume-renderer_amd/slice_context.py is the normative
// arithmetic): a slice frame in which the unshaded emission-absorption march runs from the ray's entry into the box up to the winning
// slice, and the opaque slice is composited behind it.  Nothing is restated that exists: the slice stage, the slab's walk and the plane's tap are
// ovr_hip_slices.h's functions (slice_stage, slice_ray), the tap, the transfer function in LDS (stage_tf, tf_coord, tf_alpha, tf_color), the opacity correction
// and the quad helpers are ovr_hip_device.h's, called as raymarch_kernel calls them.
//
// One kernel, slice_context_kernel<VT, AM, ORTHO>, for plane-only and slab sets alike, in the in-place march's place in the launch sequence; it exists with the
// clipped box test alone (a frame without a clip box runs it with the unit box, whose bounds give the unclipped test's bits - DESIGN.md section 12), for both
// cameras.  Four lanes per ray; a round is kProjectK x 4 steps - four gather instructions in flight per lane, the unshaded in-place march's round.  Every
// lane of a quad runs the ray's (tx, ty) recurrence and, over each round, the alpha / colour recurrence in step order with the other lanes' opacities and
// colours fetched by DPP quad broadcasts; the loop condition (ty > tx and alpha < 0.9999) is tested before every step, so the counters are the march's.
// With no slice met the cut is t1 and the arithmetic IS raymarch_kernel<VT, 0, AM, false, false>'s, operation for operation (x * 1 is exact): such a frame
// equals the SHADE_NONE march frame bit for bit (tests/test_slice_context_gpu.py holds the two kernels against each other).
// The slice behind the context is sampled only by quads whose ray is unsaturated: slice_ray is handed hit = false for the others, so a saturated ray neither
// taps a plane nor walks a slab.
#pragma once

#include "ovr_hip_slices.h"

namespace ovrhip {

struct SliceContextResult {   // quad-uniform but for the two counters
  int k;                      // the composited slice's index + 1; 0: none (nothing met, or the ray saturated in front of it)
  float v, key;               // the composited slice's value and t_k
  unsigned int steps;         // context steps taken (the ray's)
  float alpha;                // the sample's alpha, the slice included
  f3 color;                   // premultiplied
  unsigned int fetched, shaded; // THIS LANE's: context steps fetched + the composited winner's taps; context steps with a' > 0
};

template <int VT, int AM>
__device__ __forceinline__ SliceContextResult slice_context_ray(const RayMarchParams& P, const VolConsts& vc, const TfConsts& tf, const MarchConsts& mc, f3 org, f3 dir,
                                                                float t0, float t1, bool hit, const SubMask& subm)
{
  constexpr int K = kProjectK;
  const int sub = subm.sub;
  const float scale = P.slice_context_scale; // wave-uniform: a scalar register
  // ---- the cut: the winner's key, if it counts as met under the slice frame's rule (a slab needs a step: slice_walk's first validity bit)
  const SliceMeet w = slice_stage(P, org, dir, t0, t1, hit);
  const bool met = w.k >= 0 && (w.mode == 0 || fminf(w.tb, w.ta + mc.step) > w.ta);
  const float tc = met ? w.key : t1;
  // ---- the context march: raymarch_kernel's unshaded in-place rounds with tc in t1's place
  float alpha = 0.f;
  f3 color = mk3(0, 0, 0);
  unsigned int n_samples = 0, n_shaded = 0;
  bool live = hit;
  float tx = t0, ty = fminf(tc, t0 + mc.step);
  while (__ballot(live) != 0ull) {
    // the ray's next 4K steps: every lane runs the (tx, ty) recurrence, keeps its own K steps and one validity bit per step
    unsigned int vmask = 0;
    Tap taps[K];
    float dts[K], tms[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float txq[4], tyq[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        txq[b] = tx; tyq[b] = ty;
        vmask |= (ty > tx) ? (1u << (4 * k + b)) : 0u;
        tx = ty;
        ty = fminf(tx + mc.step, tc);
      }
      const float mtx = sel4(txq[0], txq[1], txq[2], txq[3], subm);
      const float mty = sel4(tyq[0], tyq[1], tyq[2], tyq[3], subm);
      dts[k] = mty - mtx;
      tms[k] = 0.5f * (mtx + mty);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const f3 pos = mk3(fmaf(tms[k], dir.x, org.x), fmaf(tms[k], dir.y, org.y), fmaf(tms[k], dir.z, org.z));
      tap_coords(vc, to_object(mc, pos), taps[k]);
    }
    // branch-free, like the march: dead lanes load (their coordinates are clamped, the loads are in bounds) and feed a = 0
#pragma unroll
    for (int k = 0; k < K; ++k) tap_loads<VT, AM>(vc, taps[k]);
    // own samples: value, TF coordinate, corrected and scaled opacity
    float va[K], aa[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      va[k] = tf_coord(tf, tap_finish<VT>(vc, taps[k]));
      aa[k] = opacity_correction<false>(tf_alpha<true>(tf, va[k]), mc.base * dts[k]) * scale;
    }
    // transparent round (wave-uniform): no live sample of any ray of the wave has opacity > 0 - every step adds exactly 0; only liveness and the counter move
    {
      bool opaque = false;
#pragma unroll
      for (int k = 0; k < K; ++k) opaque = opaque || (aa[k] > 0.f);
      if (__ballot(opaque && live) == 0ull) {
        const bool go = live && (alpha < 0.9999f);
#pragma unroll
        for (int k = 0; k < K; ++k) n_samples += (go && ((vmask >> (4 * k + sub)) & 1u) != 0u) ? 1u : 0u;
        live = go && ((vmask >> (4 * K - 1)) & 1u) != 0u;
        continue;
      }
    }
    f3 ca[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const f3 rgb = tf_color(tf, va[k]);
      ca[k] = mk3(clamp01(rgb.x), clamp01(rgb.y), clamp01(rgb.z));
    }
    // the ray's recurrence over the 4K steps, in order; every lane of the quad computes all of it (a dead step feeds a = 0: fma(tr, 0, x) == x exactly)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      bool lv[4]; // the loop condition at each step
#define OVR_STEP(B)                                                                                                            \
      {                                                                                                                        \
        const float aj = quad_bcast<B>(aa[k]);                                                                                 \
        live = live && ((vmask >> (4 * k + B)) & 1u) != 0u && (alpha < 0.9999f);                                               \
        lv[B] = live;                                                                                                          \
        const float ae = live ? aj : 0.f;                                                                                      \
        const float trj = 1.f - alpha;                                                                                         \
        const float cxj = quad_bcast<B>(ca[k].x), cyj = quad_bcast<B>(ca[k].y), czj = quad_bcast<B>(ca[k].z);                  \
        color.x = fmaf(trj * cxj, ae, color.x);                                                                                \
        color.y = fmaf(trj * cyj, ae, color.y);                                                                                \
        color.z = fmaf(trj * czj, ae, color.z);                                                                                \
        alpha = fmaf(trj, ae, alpha);                                                                                          \
      }
      OVR_STEP(0) OVR_STEP(1) OVR_STEP(2) OVR_STEP(3)
#undef OVR_STEP
      const bool mlive = sub == 0 ? lv[0] : sub == 1 ? lv[1] : sub == 2 ? lv[2] : lv[3];
      n_samples += mlive ? 1u : 0u;
      n_shaded += (mlive && aa[k] > 0.f) ? 1u : 0u;
    }
  }
  SliceContextResult r;
  {
    const float o = __uint_as_float(n_samples);
    r.steps = __float_as_uint(quad_bcast<0>(o)) + __float_as_uint(quad_bcast<1>(o)) + __float_as_uint(quad_bcast<2>(o)) + __float_as_uint(quad_bcast<3>(o));
  }
  // ---- the slice behind it: composited iff one is met and the ray is unsaturated - the loop's own condition.  slice_ray meets nothing without `hit`
  const SliceResult sr = slice_ray<VT, AM, false>(P, vc, mc, org, dir, t0, t1, hit && met && alpha < 0.9999f, subm);
  r.k = sr.k;
  r.v = sr.k > 0 ? sr.v : 0.f;
  r.key = sr.k > 0 ? sr.key : 0.f;
  if (sr.k > 0) {
    const f3 c = isosurface_colour(P, sr.v); // the slice frame's colour: the alpha table is not read, a slice is opaque
    const float tr = 1.f - alpha;
    color.x = fmaf(tr * c.x, 1.f, color.x);
    color.y = fmaf(tr * c.y, 1.f, color.y);
    color.z = fmaf(tr * c.z, 1.f, color.z);
    alpha = fmaf(tr, 1.f, alpha);
  }
  r.alpha = alpha;
  r.color = color;
  r.fetched = n_samples + (sr.k > 0 ? sr.fetched : 0u);
  r.shaded = n_shaded;
  return r;
}

// LDS: [axis tables][TF colour][TF alpha], the march's carve without its request queues (plan_slices sizes it)
template <int VT, int AM>
__device__ __forceinline__ void slice_context_stage(const RayMarchParams& P, unsigned char* lds_raw, VolConsts& vc, TfConsts& tf)
{
  const size_t tb = (stage_tables<VT, AM>(P, lds_raw, vc) + 15) & ~(size_t)15;
  stage_tf(P, lds_raw + tb, true, tf); // (ends on a barrier)
}

// a context frame: slice_walk_kernel's frame around slice_context_ray; the pixel is the march's un-premultiplied one, the buffer mapframe hands out as `grad`
// carries the slice layer (v, t_k, k + 1) of the composited slice.  The register budget is the march's: at most 3 waves per SIMD, so that the compiler keeps
// the round's K tap groups in flight instead of serialising them for a 4th wave
template <int VT, int AM, bool ORTHO = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, kMarchWavesPerEu))) void slice_context_kernel(const RayMarchParams P)
{
  static_assert(slice_variant_exists(true, AM, false, true, ORTHO, true) && (AM != 4 || RowLoads<VT, 4>::on), "no such variant of the slice context kernel (host/launch_plan.hpp)");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & 3;
  const bool owner = sub == 0;
  const SubMask subm = make_submask(sub);
  int ix, iy;
  const bool active = assign_pixel_quad(P, lane, wave, ix, iy);
  VolConsts vc;
  MarchConsts mc;
  setup_consts(P, vc, mc);
  TfConsts tf;
  const bool staged = __syncthreads_or(active ? 1 : 0) != 0; // workgroup-uniform
  if (staged) slice_context_stage<VT, AM>(P, lds_raw, vc, tf);
  else {
    tf = TfConsts{};
    vc.tab_x = vc.tab_y = vc.tab_z = nullptr;
    vc.tab_z64 = nullptr;
  }
  unsigned int n_rays = 0, n_samples = 0, n_shaded = 0, n_outside_hits = 0;
  const float rsx = 1.f / (float)P.width, rsy = 1.f / (float)P.height;
  const float scx = ((float)ix + .5f) * rsx, scy = ((float)iy + .5f) * rsy;
  const unsigned int pixel_index = (unsigned int)ix + (unsigned int)iy * (unsigned int)P.width;
  unsigned int v0 = (unsigned int)P.frame_index, v1 = pixel_index; // RandomTEA(frame_index, pixel_index)
  float o_a = 0.f;
  f3 o_c = mk3(0, 0, 0), o_g = mk3(0, 0, 0);
  for (int k_spp = 0; k_spp < P.spp; ++k_spp) { // uniform trip count
    float sx, sy;
    slice_sample_position(P, ix, iy, k_spp, scx, scy, rsx, rsy, v0, v1, sx, sy);
    const float ux = sx - 0.5f, uy = sy - 0.5f;
    f3 org, dir;
    pixel_ray<ORTHO>(P, ux, uy, org, dir);
    const f3 oo = to_object(mc, org);
    const f3 od = mk3(dir.x * mc.inv_scale.x, dir.y * mc.inv_scale.y, dir.z * mc.inv_scale.z);
    float t0 = 0.f, t1 = FLT_MAX;
    const bool live = active && primary_box_test<true, ORTHO>(P, t0, t1, oo, od); // (active implies staged)
    if (active && owner) ++n_rays;
    if (live && owner && box_ignored_slab_outside<true>(P, oo, od)) ++n_outside_hits;
    const SliceContextResult cr = slice_context_ray<VT, AM>(P, vc, tf, mc, org, dir, t0, t1, live, subm);
    n_samples += cr.fetched;
    n_shaded += cr.shaded;
    // the march's pixel sample: alpha_blend with an always-missing background
    o_a += cr.alpha;
    if (cr.alpha > 0.f) { o_c.x += cr.color.x / cr.alpha; o_c.y += cr.color.y / cr.alpha; o_c.z += cr.color.z / cr.alpha; }
    if (cr.k > 0) { o_g.x += cr.v; o_g.y += cr.key; o_g.z += (float)cr.k; }
  }
  if (active && owner) {
    const float rspp = 1.f / (float)P.spp;
    o_a *= rspp;
    o_c.x *= rspp; o_c.y *= rspp; o_c.z *= rspp;
    o_g.x *= rspp; o_g.y *= rspp; o_g.z *= rspp;
    write_pixel(P, pixel_index, o_c, o_a, o_g);
  }
  store_block_counters(P, reinterpret_cast<unsigned int*>(lds_raw), lane, wave, n_rays, n_samples, n_shaded, 0u, (active && owner) ? 1u : 0u, 0u, 0u, n_outside_hits);
}

// the known-answer entry's kernel: ray i = the quad of lanes 4 i ... 4 i + 3, through slice_context_ray as the frame's kernel calls it.
// out: (k + 1 or 0, v, t_k, context steps taken, r, g, b, a of the pixel sample) per ray
template <int VT, int AM>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, kMarchWavesPerEu))) void slice_context_floats_kernel(const RayMarchParams P, const float* org, const float* dir, float* out, long long n)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int sub = threadIdx.x & 3;
  const SubMask subm = make_submask(sub);
  VolConsts vc;
  MarchConsts mc;
  setup_consts(P, vc, mc);
  TfConsts tf;
  slice_context_stage<VT, AM>(P, lds_raw, vc, tf);
  const long long i = ((long long)blockIdx.x * kBlock + threadIdx.x) >> 2;
  const bool valid = i < n;
  const long long j = valid ? i : 0;
  const f3 o = mk3(org[3 * j], org[3 * j + 1], org[3 * j + 2]), d = mk3(dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]);
  const f3 oo = to_object(mc, o), od = mk3(d.x * mc.inv_scale.x, d.y * mc.inv_scale.y, d.z * mc.inv_scale.z);
  float t0 = 0.f, t1 = FLT_MAX;
  const bool live = valid && box_test<true>(P, t0, t1, oo, od);
  const SliceContextResult cr = slice_context_ray<VT, AM>(P, vc, tf, mc, o, d, t0, t1, live, subm);
  if (valid && sub == 0) {
    const bool lit = cr.alpha > 0.f;
    float* q = out + 8 * i;
    q[0] = (float)cr.k; q[1] = cr.v; q[2] = cr.key; q[3] = (float)cr.steps;
    q[4] = lit ? cr.color.x / cr.alpha : 0.f; q[5] = lit ? cr.color.y / cr.alpha : 0.f; q[6] = lit ? cr.color.z / cr.alpha : 0.f; q[7] = cr.alpha;
  }
}

typedef void (*SliceContextFloatsKernel)(const RayMarchParams, const float*, const float*, float*, long long);
struct SliceContextKernels { FrameKernel frame = nullptr; SliceContextFloatsKernel floats = nullptr; }; // nullptr: no such variant of this type
// the variants: the camera kind alone
template <int VT, int AM> struct SliceContextVariants {
  template <unsigned I> static constexpr SliceContextKernels at()
  {
    if constexpr (!slice_variant_exists(true, AM, false, true, I != 0, true)) return {};
    else return { slice_context_kernel<VT, AM, I != 0>, slice_context_floats_kernel<VT, AM> };
  }
};
// a context plan's kernels of a voxel type; nullptr for a replica's type (or mode 4 on a layout without row loads), like slice_kernels_of
template <int VT>
SliceContextKernels slice_context_kernels_of(const LaunchPlan& pl)
{
  if (pl.error || !pl.slices.on || !pl.slices.context || !pl.slices.clipped || pl.slices.skip) return SliceContextKernels();
  const unsigned i = pl.orthographic ? 1u : 0u;
  return dispatch_addressing<SliceContextKernels, VT, true>(pl.am, [&](auto m) { return variant_at<SliceContextVariants<VT, decltype(m)::value>>(i, std::make_integer_sequence<unsigned, 2>()); });
}

} // namespace ovrhip
