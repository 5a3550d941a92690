// ovr_hip_max_depth.h - the depth limit (include/ovr_hip.h ovr_hip_set_max_depth; open-volume-renderer_amd/max_depth.py is the normative arithmetic;
// DESIGN.md section 26): the march that ends every ray of a pixel on a ray parameter the caller hands in, so that the frame is what lies in front of the
// caller's opaque geometry.  Nothing is restated that exists: the tap, the transfer function in LDS (stage_tf, tf_coord, tf_alpha, tf_color), the opacity
// correction, the shade factor (shade_light, shade_factor) and the quad helpers are ovr_hip_device.h's; the frame shell, the (tx, ty) recurrence with a cut in
// t1's place, the loop test before every step and the transparent-round shortcut are the slice context kernel's; the forward difference
// (gradient_difference), the ballots around the gradient taps and the shaded branch are the gradient-opacity kernel's.
//
// max_depth_kernel<VT, AM, SHADE, ORTHO> stands in the in-place march's place in the launch sequence; it exists with the clipped box test alone (a frame
// without a clip box runs it with the unit box, whose bounds give the unclipped test's bits - DESIGN.md section 12), for shading NONE (SHADE = 0) and GRADIENT
// (SHADE = 1) and both cameras.  Four lanes per ray; a round is kProjectK x 4 steps.  One depth load per pixel, in front of the samples' loop: every sample of
// the pixel takes it.  With z = +inf (or NaN, or z >= t1) the cut is t1 and every operation is the march's: the frame is the march's bit for bit.
#pragma once

#include "ovr_hip_gradient_opacity.h" // (gradient_difference; through it ovr_hip_slices.h, the frame shell: slice_sample_position)

namespace ovrhip {

struct MaxDepthResult { // quad-uniform but for the lane counters
  unsigned int steps;   // steps taken (the ray's)
  unsigned int opaque;  // of them, steps with corrected opacity > 0
  float tx;             // tx at exit: the back end of the last step taken, t0 without one
  float alpha;
  f3 color, gradient;   // premultiplied
  unsigned int fetched, shaded; // THIS LANE's: steps taken; steps with a > 0
};

// the cut of a pixel sample: z < +inf is false for +inf and for NaN - no surface at this pixel
__device__ __forceinline__ float max_depth_cut(float t1, float z)
{
  const bool limited = z < __builtin_inff();
  return limited ? fminf(t1, z) : t1;
}

// the march's loop from t0 up to the cut tc (tc <= t1; tc <= t0 takes no step)
template <int VT, int AM, int SHADE, bool ORTHO>
__device__ __forceinline__ MaxDepthResult max_depth_ray(const RayMarchParams& P, const VolConsts& vc, const TfConsts& tf, const MarchConsts& mc, f3 org, f3 dir,
                                                        float t0, float tc, bool hit, const SubMask& subm)
{
  constexpr int K = kProjectK;
  const int sub = subm.sub;
  float alpha = 0.f;
  f3 color = mk3(0, 0, 0), gradient = mk3(0, 0, 0);
  unsigned int n_samples = 0, n_shaded = 0;
  bool live = hit;
  float tx = t0, ty = fminf(tc, t0 + mc.step);
  float t_exit = t0;
  while (__ballot(live) != 0ull) {
    // the ray's next 4K steps: every lane runs the (tx, ty) recurrence, keeps its own K steps and one validity bit per step
    unsigned int vmask = 0;
    Tap taps[K];
    f3 poss[K];
    float dts[K], tms[K], tys[K];
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
      tys[k] = mty;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      poss[k] = mk3(fmaf(tms[k], dir.x, org.x), fmaf(tms[k], dir.y, org.y), fmaf(tms[k], dir.z, org.z));
      tap_coords(vc, to_object(mc, poss[k]), taps[k]);
    }
    // branch-free, like the march: dead lanes load (their coordinates are clamped, the loads are in bounds) and feed a = 0
#pragma unroll
    for (int k = 0; k < K; ++k) tap_loads<VT, AM>(vc, taps[k]);
    // own samples: value, TF coordinate, corrected opacity
    float sa[K], va[K], aa[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      sa[k] = tap_finish<VT>(vc, taps[k]);
      va[k] = tf_coord(tf, sa[k]);
      aa[k] = opacity_correction<false>(tf_alpha<true>(tf, va[k]), mc.base * dts[k]);
    }
    // transparent round (wave-uniform): no live sample of any ray of the wave has opacity > 0 - every step adds exactly 0; only liveness and the counters move
    {
      bool opaque = false;
#pragma unroll
      for (int k = 0; k < K; ++k) opaque = opaque || (aa[k] > 0.f);
      if (__ballot(opaque && live) == 0ull) {
        const bool go = live && (alpha < 0.9999f);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const bool mlive = go && ((vmask >> (4 * k + sub)) & 1u) != 0u;
          n_samples += mlive ? 1u : 0u;
          t_exit = mlive ? tys[k] : t_exit;
        }
        live = go && ((vmask >> (4 * K - 1)) & 1u) != 0u;
        continue;
      }
    }
    // colours; under GRADIENT the forward difference, the shade factor and the camera normal of the steps with opacity, behind a wave-uniform ballot: the
    // taps' coordinates are clamped, the lanes of the wave that do not need the step's gradient load in bounds and drop the result
    f3 ca[K], na[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const f3 rgb = tf_color(tf, va[k]);
      na[k] = mk3(0, 0, 0);
      if (SHADE == 0) ca[k] = mk3(clamp01(rgb.x), clamp01(rgb.y), clamp01(rgb.z));
      else {
        ca[k] = mk3(0, 0, 0);
        if (__ballot(aa[k] > 0.f && live) != 0ull) {
          const f3 gn = normalize3(gradient_difference<VT, AM>(vc, mc, to_object(mc, poss[k]), sa[k]));
          const f3 n_o = mk3(-gn.x, -gn.y, -gn.z);
          const f3 n_w = normalize3(mk3(n_o.x * mc.otw_it.x, n_o.y * mc.otw_it.y, n_o.z * mc.otw_it.z));
          f3 n_c = mk3(0, 0, 0);
          if (P.grad) {
            const float* m = P.wtc_it;
            n_c = normalize3(mk3(fmaf(n_w.x, m[0], fmaf(n_w.y, m[3], n_w.z * m[6])), fmaf(n_w.x, m[1], fmaf(n_w.y, m[4], n_w.z * m[7])),
                                 fmaf(n_w.x, m[2], fmaf(n_w.y, m[5], n_w.z * m[8]))));
          }
          const float shade = shade_factor<true>(P, shade_light<true, ORTHO>(P, mc.light, n_w, poss[k]), 0.f);
          ca[k] = mk3(clamp01(rgb.x * shade), clamp01(rgb.y * shade), clamp01(rgb.z * shade)); // (clamp01 maps the NaN of a zero gradient to 0)
          na[k] = mk3(clamp01(n_c.x), clamp01(n_c.y), clamp01(n_c.z));
        }
      }
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
        if (SHADE != 0) {                                                                                                      \
          const float nxj = quad_bcast<B>(na[k].x), nyj = quad_bcast<B>(na[k].y), nzj = quad_bcast<B>(na[k].z);                \
          gradient.x = fmaf(trj * nxj, ae, gradient.x);                                                                        \
          gradient.y = fmaf(trj * nyj, ae, gradient.y);                                                                        \
          gradient.z = fmaf(trj * nzj, ae, gradient.z);                                                                        \
        }                                                                                                                      \
        alpha = fmaf(trj, ae, alpha);                                                                                          \
      }
      OVR_STEP(0) OVR_STEP(1) OVR_STEP(2) OVR_STEP(3)
#undef OVR_STEP
      const bool mlive = sub == 0 ? lv[0] : sub == 1 ? lv[1] : sub == 2 ? lv[2] : lv[3];
      n_samples += mlive ? 1u : 0u;
      n_shaded += (mlive && aa[k] > 0.f) ? 1u : 0u;
      t_exit = mlive ? tys[k] : t_exit;
    }
  }
  MaxDepthResult r;
  {
    const float o = __uint_as_float(n_samples), s = __uint_as_float(n_shaded);
    r.steps = __float_as_uint(quad_bcast<0>(o)) + __float_as_uint(quad_bcast<1>(o)) + __float_as_uint(quad_bcast<2>(o)) + __float_as_uint(quad_bcast<3>(o));
    r.opaque = __float_as_uint(quad_bcast<0>(s)) + __float_as_uint(quad_bcast<1>(s)) + __float_as_uint(quad_bcast<2>(s)) + __float_as_uint(quad_bcast<3>(s));
    r.tx = fmaxf(fmaxf(quad_bcast<0>(t_exit), quad_bcast<1>(t_exit)), fmaxf(quad_bcast<2>(t_exit), quad_bcast<3>(t_exit))); // (ty only grows along a ray)
  }
  r.alpha = alpha;
  r.color = color;
  r.gradient = gradient;
  r.fetched = n_samples;
  r.shaded = n_shaded;
  return r;
}

// a depth-limited frame: the slice context kernel's frame around max_depth_ray; the pixel is the march's un-premultiplied one of what lies in front of the
// cut, the gradient layer the shaded march's (zero under shading NONE).  LDS: [axis tables][TF colour][TF alpha] - slice_context_stage's carve.  The register
// budget is the march's.  P.max_depth holds P.width x P.height values (the host draws the frame only then): the load's index is the index write_pixel writes at
template <int VT, int AM, int SHADE, bool ORTHO = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, kMarchWavesPerEu))) void max_depth_kernel(const RayMarchParams P)
{
  static_assert(max_depth_variant_exists(SHADE, AM, false, true, ORTHO) && (AM != 4 || RowLoads<VT, 4>::on), "no such variant of the depth-limited kernel (host/launch_plan.hpp)");
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
  if (staged) {
    const size_t tb = (stage_tables<VT, AM>(P, lds_raw, vc) + 15) & ~(size_t)15;
    stage_tf(P, lds_raw + tb, true, tf); // (ends on a barrier)
  }
  else {
    tf = TfConsts{};
    vc.tab_x = vc.tab_y = vc.tab_z = nullptr;
    vc.tab_z64 = nullptr;
  }
  unsigned int n_rays = 0, n_samples = 0, n_shaded = 0, n_outside_hits = 0;
  const float rsx = 1.f / (float)P.width, rsy = 1.f / (float)P.height;
  const float scx = ((float)ix + .5f) * rsx, scy = ((float)iy + .5f) * rsy;
  const unsigned int pixel_index = (unsigned int)ix + (unsigned int)iy * (unsigned int)P.width;
  const float z = active ? P.max_depth[pixel_index] : __builtin_inff(); // the pixel's: every sample takes it
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
    const MaxDepthResult mr = max_depth_ray<VT, AM, SHADE, ORTHO>(P, vc, tf, mc, org, dir, t0, max_depth_cut(t1, z), live, subm);
    n_samples += mr.fetched;
    n_shaded += mr.shaded;
    // the march's pixel sample: alpha_blend with an always-missing background
    o_a += mr.alpha;
    if (mr.alpha > 0.f) {
      o_c.x += mr.color.x / mr.alpha; o_c.y += mr.color.y / mr.alpha; o_c.z += mr.color.z / mr.alpha;
      o_g.x += mr.gradient.x / mr.alpha; o_g.y += mr.gradient.y / mr.alpha; o_g.z += mr.gradient.z / mr.alpha;
    }
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

// the known-answer entry's kernel: ray i = the quad of lanes 4 i ... 4 i + 3, ending on depth[i], through max_depth_ray as the frame's kernel calls it (the
// perspective camera's view vector: the rays are the caller's).  out: (steps taken, the cut tc, tx at exit, steps with a > 0, r, g, b, a of the pixel sample)
// per ray
template <int VT, int AM, int SHADE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, kMarchWavesPerEu))) void max_depth_floats_kernel(const RayMarchParams P, const float* org, const float* dir, const float* depth, float* out, long long n)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int sub = threadIdx.x & 3;
  const SubMask subm = make_submask(sub);
  VolConsts vc;
  MarchConsts mc;
  setup_consts(P, vc, mc);
  TfConsts tf;
  {
    const size_t tb = (stage_tables<VT, AM>(P, lds_raw, vc) + 15) & ~(size_t)15;
    stage_tf(P, lds_raw + tb, true, tf); // (ends on a barrier)
  }
  const long long i = ((long long)blockIdx.x * kBlock + threadIdx.x) >> 2;
  const bool valid = i < n;
  const long long j = valid ? i : 0;
  const f3 o = mk3(org[3 * j], org[3 * j + 1], org[3 * j + 2]), d = mk3(dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]);
  const f3 oo = to_object(mc, o), od = mk3(d.x * mc.inv_scale.x, d.y * mc.inv_scale.y, d.z * mc.inv_scale.z);
  float t0 = 0.f, t1 = FLT_MAX;
  const bool live = valid && box_test<true>(P, t0, t1, oo, od);
  const float tc = max_depth_cut(t1, depth[j]);
  const MaxDepthResult mr = max_depth_ray<VT, AM, SHADE, false>(P, vc, tf, mc, o, d, t0, tc, live, subm);
  if (valid && sub == 0) {
    const bool lit = mr.alpha > 0.f;
    float* q = out + 8 * i;
    q[0] = (float)mr.steps; q[1] = live ? tc : 0.f; q[2] = live ? mr.tx : 0.f; q[3] = (float)mr.opaque;
    q[4] = lit ? mr.color.x / mr.alpha : 0.f; q[5] = lit ? mr.color.y / mr.alpha : 0.f; q[6] = lit ? mr.color.z / mr.alpha : 0.f; q[7] = mr.alpha;
  }
}

typedef void (*MaxDepthFloatsKernel)(const RayMarchParams, const float*, const float*, const float*, float*, long long);
struct MaxDepthKernels { FrameKernel frame = nullptr; MaxDepthFloatsKernel floats = nullptr; }; // nullptr: no such variant of this type
// the variants: bit 0 the camera kind, bit 1 the shading mode
template <int VT, int AM> struct MaxDepthVariants {
  template <unsigned I> static constexpr MaxDepthKernels at()
  {
    if constexpr (!max_depth_variant_exists((I >> 1) & 1, AM, false, true, (I & 1u) != 0)) return {};
    else return { max_depth_kernel<VT, AM, (I >> 1) & 1, (I & 1u) != 0>, max_depth_floats_kernel<VT, AM, (I >> 1) & 1> };
  }
};
// a depth-limited plan's kernels of a voxel type; nullptr for a replica's type (or mode 4 on a layout without row loads), like slice_context_kernels_of
template <int VT>
MaxDepthKernels max_depth_kernels_of(const LaunchPlan& pl)
{
  if (pl.error || !pl.max_depth.on || !pl.max_depth.clipped || pl.skip) return MaxDepthKernels();
  const unsigned i = (pl.orthographic ? 1u : 0u) | (pl.max_depth.shade ? 2u : 0u);
  return dispatch_addressing<MaxDepthKernels, VT, true>(pl.am, [&](auto m) { return variant_at<MaxDepthVariants<VT, decltype(m)::value>>(i, std::make_integer_sequence<unsigned, 4>()); });
}

} // namespace ovrhip
