// ovr_hip_gradient_opacity.h - gradient opacity (include/ovr_hip.h ovr_hip_set_gradient_opacity; open-volume-renderer_amd/gradient_opacity.py is the
// normative arithmetic): the march in which the transfer function's opacity of every sample is weighted by a ramp over the magnitude of
// the local gradient, so that the inside of a material fades and its boundaries stay.  Nothing is restated that exists: the tap, the transfer function in LDS
// (stage_tf, tf_coord, tf_alpha, tf_color), the opacity correction, the shade factor (shade_light, shade_factor) and the quad helpers are ovr_hip_device.h's,
// called as raymarch_kernel and shade_request call them; the frame shell, the (tx, ty) recurrence, the loop test before every step and the transparent-round
// shortcut are the slice context kernel's.  The forward difference is shade_request's, restated here (gradient_difference) because shade_request forms it
// inside its request: with the neutral ramp (-1, 0) a GRADIENT-shaded frame is the shaded march's bit for bit, which is the test that the two agree
// (tests/test_gradient_opacity_gpu.py).
//
// gradient_opacity_kernel<VT, AM, SHADE, ORTHO> stands in the in-place march's place in the launch sequence; it exists with the clipped box test alone (a frame
// without a clip box runs it with the unit box, whose bounds give the unclipped test's bits - DESIGN.md section 12), for shading NONE (SHADE = 0) and GRADIENT
// (SHADE = 1) and both cameras.  Four lanes per ray; a round is kProjectK x 4 steps.  The three gradient taps of a step are issued together, for the steps whose
// table opacity is > 0, behind wave-uniform ballots: a wave crossing transparent data pays nothing for them.  The shaded branch - normal, shade factor, camera
// normal - sits behind a second ballot on the corrected opacity.  Material and light are kernel arguments (shade_light<true>): the reference's values give the
// reference's bits.
#pragma once

#include "ovr_hip_slices.h" // (the frame shell: slice_sample_position)

namespace ovrhip {

struct GradientOpacityResult { // quad-uniform but for the lane counters
  unsigned int steps;          // steps taken (the ray's)
  unsigned int gradients;      // of them, steps that fetched a gradient (table opacity > 0)
  unsigned int opaque;         // of them, steps with corrected, weighted opacity > 0
  float tx;                    // tx at exit: the back end of the last step taken, t0 without one
  float alpha;
  f3 color, gradient;          // premultiplied
  unsigned int fetched, shaded; // THIS LANE's: steps taken; steps with a > 0
};

// shade_request's forward difference at the object position po with the sample s there: one-sided, flipped at the upper bound, the three taps issued together
template <int VT, int AM>
__device__ __forceinline__ f3 gradient_difference(const VolConsts& vc, const MarchConsts& mc, f3 po, float s)
{
  const bool flx = (po.x + mc.gstep.x) > 1.f, fly = (po.y + mc.gstep.y) > 1.f, flz = (po.z + mc.gstep.z) > 1.f;
  const f3 pgx = mk3(po.x + (flx ? -mc.gstep.x : mc.gstep.x), po.y, po.z), pgy = mk3(po.x, po.y + (fly ? -mc.gstep.y : mc.gstep.y), po.z);
  const f3 pgz = mk3(po.x, po.y, po.z + (flz ? -mc.gstep.z : mc.gstep.z));
  Tap tgx, tgy, tgz;
  tap_issue<VT, AM>(vc, pgx, tgx);
  tap_issue<VT, AM>(vc, pgy, tgy);
  tap_issue<VT, AM>(vc, pgz, tgz);
  const float sgx = tap_finish<VT>(vc, tgx), sgy = tap_finish<VT>(vc, tgy), sgz = tap_finish<VT>(vc, tgz);
  f3 g;
#if OVR_PARITY_EXACT
  g.x = (sgx - s) / (flx ? -mc.gstep.x : mc.gstep.x);
  g.y = (sgy - s) / (fly ? -mc.gstep.y : mc.gstep.y);
  g.z = (sgz - s) / (flz ? -mc.gstep.z : mc.gstep.z);
#else
  g.x = (sgx - s) * (flx ? -mc.ginv.x : mc.ginv.x);
  g.y = (sgy - s) * (fly ? -mc.ginv.y : mc.ginv.y);
  g.z = (sgz - s) * (flz ? -mc.ginv.z : mc.ginv.z);
#endif
  return g;
}

// the weight of a sample whose object-space gradient is g: the world gradient's length in transfer-function ranges per world unit length, through the ramp.
// sqrtf is the correctly rounded root in both builds
__device__ __forceinline__ float gradient_opacity_weight(const RayMarchParams& P, const TfConsts& tf, const MarchConsts& mc, f3 g)
{
  const f3 w = mk3(g.x * mc.inv_scale.x, g.y * mc.inv_scale.y, g.z * mc.inv_scale.z);
  const float m = sqrtf(dot3(w, w)) * tf.scale;
  return clamp01((m - P.gradop_lo) * P.gradop_inv_ramp);
}

template <int VT, int AM, int SHADE, bool ORTHO>
__device__ __forceinline__ GradientOpacityResult gradient_opacity_ray(const RayMarchParams& P, const VolConsts& vc, const TfConsts& tf, const MarchConsts& mc, f3 org, f3 dir,
                                                                      float t0, float t1, bool hit, const SubMask& subm)
{
  constexpr int K = kProjectK;
  const int sub = subm.sub;
  float alpha = 0.f;
  f3 color = mk3(0, 0, 0), gradient = mk3(0, 0, 0);
  unsigned int n_samples = 0, n_shaded = 0, n_gradients = 0;
  bool live = hit;
  float tx = t0, ty = fminf(t1, t0 + mc.step);
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
        ty = fminf(tx + mc.step, t1);
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
    // own samples: value, TF coordinate, table opacity
    float sa[K], va[K], aa[K];
    unsigned int gmask = 0; // own steps that fetch a gradient
#pragma unroll
    for (int k = 0; k < K; ++k) {
      sa[k] = tap_finish<VT>(vc, taps[k]);
      va[k] = tf_coord(tf, sa[k]);
      aa[k] = tf_alpha<true>(tf, va[k]);
      gmask |= aa[k] > 0.f ? (1u << k) : 0u;
    }
    // the gradients: only where a live step of the wave has table opacity (a_tf * w is 0 whatever w where a_tf is 0).  The taps' coordinates are clamped:
    // the lanes of the wave that do not need the step's gradient load in bounds and drop the result
    f3 ga[K];
#pragma unroll
    for (int k = 0; k < K; ++k) ga[k] = mk3(0, 0, 0);
    if (__ballot(gmask != 0u && live) != 0ull) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const bool need = ((gmask >> k) & 1u) != 0u;
        if (__ballot(need && live) != 0ull) {
          const f3 g = gradient_difference<VT, AM>(vc, mc, to_object(mc, poss[k]), sa[k]);
          const float w = gradient_opacity_weight(P, tf, mc, g);
          ga[k] = g;
          aa[k] = need ? aa[k] * w : aa[k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) aa[k] = opacity_correction<false>(aa[k], mc.base * dts[k]);
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
          n_gradients += (mlive && ((gmask >> k) & 1u) != 0u) ? 1u : 0u;
          t_exit = mlive ? tys[k] : t_exit;
        }
        live = go && ((vmask >> (4 * K - 1)) & 1u) != 0u;
        continue;
      }
    }
    // colours; under GRADIENT the shade factor and the camera normal of the steps with opacity, from the gradient the weight was formed from
    f3 ca[K], na[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const f3 rgb = tf_color(tf, va[k]);
      na[k] = mk3(0, 0, 0);
      if (SHADE == 0) ca[k] = mk3(clamp01(rgb.x), clamp01(rgb.y), clamp01(rgb.z));
      else {
        ca[k] = mk3(0, 0, 0);
        if (__ballot(aa[k] > 0.f && live) != 0ull) {
          const f3 gn = normalize3(ga[k]);
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
      n_gradients += (mlive && ((gmask >> k) & 1u) != 0u) ? 1u : 0u;
      t_exit = mlive ? tys[k] : t_exit;
    }
  }
  GradientOpacityResult r;
  {
    const float o = __uint_as_float(n_samples), g = __uint_as_float(n_gradients), s = __uint_as_float(n_shaded);
    r.steps = __float_as_uint(quad_bcast<0>(o)) + __float_as_uint(quad_bcast<1>(o)) + __float_as_uint(quad_bcast<2>(o)) + __float_as_uint(quad_bcast<3>(o));
    r.gradients = __float_as_uint(quad_bcast<0>(g)) + __float_as_uint(quad_bcast<1>(g)) + __float_as_uint(quad_bcast<2>(g)) + __float_as_uint(quad_bcast<3>(g));
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

// a gradient-opacity frame: the slice context kernel's frame around gradient_opacity_ray; the pixel is the march's un-premultiplied one, the gradient layer the
// shaded march's (zero under shading NONE).  LDS: [axis tables][TF colour][TF alpha] - slice_context_stage's carve.  The register budget is the march's
template <int VT, int AM, int SHADE, bool ORTHO = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, kMarchWavesPerEu))) void gradient_opacity_kernel(const RayMarchParams P)
{
  static_assert(gradient_opacity_variant_exists(SHADE, AM, false, true, ORTHO) && (AM != 4 || RowLoads<VT, 4>::on), "no such variant of the gradient-opacity kernel (host/launch_plan.hpp)");
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
    const GradientOpacityResult gr = gradient_opacity_ray<VT, AM, SHADE, ORTHO>(P, vc, tf, mc, org, dir, t0, t1, live, subm);
    n_samples += gr.fetched;
    n_shaded += gr.shaded;
    // the march's pixel sample: alpha_blend with an always-missing background
    o_a += gr.alpha;
    if (gr.alpha > 0.f) {
      o_c.x += gr.color.x / gr.alpha; o_c.y += gr.color.y / gr.alpha; o_c.z += gr.color.z / gr.alpha;
      o_g.x += gr.gradient.x / gr.alpha; o_g.y += gr.gradient.y / gr.alpha; o_g.z += gr.gradient.z / gr.alpha;
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

// the known-answer entry's kernel: ray i = the quad of lanes 4 i ... 4 i + 3, through gradient_opacity_ray as the frame's kernel calls it (the perspective
// camera's view vector: the rays are the caller's).  out: (steps taken, of them steps that fetched a gradient, tx at exit, steps with a > 0, r, g, b, a of the
// pixel sample) per ray
template <int VT, int AM, int SHADE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, kMarchWavesPerEu))) void gradient_opacity_floats_kernel(const RayMarchParams P, const float* org, const float* dir, float* out, long long n)
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
  const GradientOpacityResult gr = gradient_opacity_ray<VT, AM, SHADE, false>(P, vc, tf, mc, o, d, t0, t1, live, subm);
  if (valid && sub == 0) {
    const bool lit = gr.alpha > 0.f;
    float* q = out + 8 * i;
    q[0] = (float)gr.steps; q[1] = (float)gr.gradients; q[2] = live ? gr.tx : 0.f; q[3] = (float)gr.opaque;
    q[4] = lit ? gr.color.x / gr.alpha : 0.f; q[5] = lit ? gr.color.y / gr.alpha : 0.f; q[6] = lit ? gr.color.z / gr.alpha : 0.f; q[7] = gr.alpha;
  }
}

typedef void (*GradientOpacityFloatsKernel)(const RayMarchParams, const float*, const float*, float*, long long);
struct GradientOpacityKernels { FrameKernel frame = nullptr; GradientOpacityFloatsKernel floats = nullptr; }; // nullptr: no such variant of this type
// the variants: bit 0 the camera kind, bit 1 the shading mode
template <int VT, int AM> struct GradientOpacityVariants {
  template <unsigned I> static constexpr GradientOpacityKernels at()
  {
    if constexpr (!gradient_opacity_variant_exists((I >> 1) & 1, AM, false, true, (I & 1u) != 0)) return {};
    else return { gradient_opacity_kernel<VT, AM, (I >> 1) & 1, (I & 1u) != 0>, gradient_opacity_floats_kernel<VT, AM, (I >> 1) & 1> };
  }
};
// a gradient-opacity plan's kernels of a voxel type; nullptr for a replica's type (or mode 4 on a layout without row loads), like slice_context_kernels_of
template <int VT>
GradientOpacityKernels gradient_opacity_kernels_of(const LaunchPlan& pl)
{
  if (pl.error || !pl.gradient_opacity.on || !pl.gradient_opacity.clipped || pl.skip) return GradientOpacityKernels();
  const unsigned i = (pl.orthographic ? 1u : 0u) | (pl.gradient_opacity.shade ? 2u : 0u);
  return dispatch_addressing<GradientOpacityKernels, VT, true>(pl.am, [&](auto m) { return variant_at<GradientOpacityVariants<VT, decltype(m)::value>>(i, std::make_integer_sequence<unsigned, 4>()); });
}

} // namespace ovrhip
