// ovr_hip_depth_output.h - the depth layer (include/ovr_hip.h ovr_hip_set_depth_output; open-volume-renderer_amd/depth_output.py is the normative arithmetic;
// DESIGN.md section 27): the march that also says WHERE along each ray its picture is - the back end of the step on which the accumulated opacity reached the
// caller's threshold tau, and the alpha-weighted sum of the steps' midpoints - in the framebuffer's second layer.  Nothing is restated that exists: the cut
// (max_depth_cut), the frame shell and the (tx, ty) recurrence are the depth-limited kernel's (ovr_hip_max_depth.h), and through it the tap, the transfer
// function in LDS, the opacity correction, the shade factor, the quad helpers and the forward difference (gradient_difference) are what they were.
//
// depth_output_kernel<VT, AM, SHADE, ORTHO> stands in the in-place march's place in the launch sequence, on the clipped box test alone, for shading NONE
// (SHADE = 0) and GRADIENT (SHADE = 1) and both cameras.  Four lanes per ray; a round is kProjectK x 4 steps.  The recurrence is max_depth_ray's with three more
// quad-uniform values - S, the ray's step count, and (reached, d, k) - and nothing in front of it: rgb, alpha, the loop test and the counters are the march's
// operation for operation, so the picture is the depth-limited frame's (without an image: the march's) bit for bit.  The gradient layer is not formed: the
// layer of a depth frame is (d, S, reached).
#pragma once

#include "ovr_hip_max_depth.h" // (max_depth_cut; through it gradient_difference and the frame shell)

namespace ovrhip {

struct DepthOutputResult { // quad-uniform but for the lane counters
  unsigned int steps;   // steps taken (the ray's)
  unsigned int opaque;  // of them, steps with corrected opacity > 0
  float tx;             // tx at exit: the back end of the last step taken, t0 without one
  float alpha;
  f3 color;             // premultiplied
  float S;              // sum of tr * tm * a over the steps taken
  float d;              // ty of the step on which alpha reached tau; 0 while not reached
  unsigned int k;       // the steps taken up to and including that one; 0 while not reached
  bool reached;
  unsigned int fetched, shaded; // THIS LANE's: steps taken; steps with a > 0
};

// the march's loop from t0 up to the cut tc (tc <= t1; tc <= t0 takes no step), with the depth accumulators beside it
template <int VT, int AM, int SHADE, bool ORTHO>
__device__ __forceinline__ DepthOutputResult depth_output_ray(const RayMarchParams& P, const VolConsts& vc, const TfConsts& tf, const MarchConsts& mc, f3 org, f3 dir,
                                                              float t0, float tc, bool hit, float tau, const SubMask& subm)
{
  constexpr int K = kProjectK;
  const int sub = subm.sub;
  float alpha = 0.f;
  f3 color = mk3(0, 0, 0);
  float S = 0.f, d = 0.f;
  unsigned int ray_steps = 0, kc = 0; // quad-uniform: every lane of the quad runs the whole recurrence
  bool reached = false;
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
    // transparent round (wave-uniform): no live sample of any ray of the wave has opacity > 0 - every step adds exactly 0 to alpha, to the colour and to S, and a
    // step with a = 0 is no crossing; only liveness, the counters and the ray's step count move
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
        ray_steps += go ? (unsigned int)__popc(vmask) : 0u; // (alpha does not move in such a round: every valid step of a ray that goes is taken)
        live = go && ((vmask >> (4 * K - 1)) & 1u) != 0u;
        continue;
      }
    }
    // colours; under GRADIENT the forward difference and the shade factor of the steps with opacity, behind a wave-uniform ballot (the camera normal of the
    // march's gradient layer is not formed: a depth frame's layer is the depth's)
    f3 ca[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const f3 rgb = tf_color(tf, va[k]);
      if (SHADE == 0) ca[k] = mk3(clamp01(rgb.x), clamp01(rgb.y), clamp01(rgb.z));
      else {
        ca[k] = mk3(0, 0, 0);
        if (__ballot(aa[k] > 0.f && live) != 0ull) {
          const f3 gn = normalize3(gradient_difference<VT, AM>(vc, mc, to_object(mc, poss[k]), sa[k]));
          const f3 n_o = mk3(-gn.x, -gn.y, -gn.z);
          const f3 n_w = normalize3(mk3(n_o.x * mc.otw_it.x, n_o.y * mc.otw_it.y, n_o.z * mc.otw_it.z));
          const float shade = shade_factor<true>(P, shade_light<true, ORTHO>(P, mc.light, n_w, poss[k]), 0.f);
          ca[k] = mk3(clamp01(rgb.x * shade), clamp01(rgb.y * shade), clamp01(rgb.z * shade)); // (clamp01 maps the NaN of a zero gradient to 0)
        }
      }
    }
    // the ray's recurrence over the 4K steps, in order; every lane of the quad computes all of it (a dead step feeds a = 0: fma(tr, 0, x) == x exactly, and
    // a = 0 is no crossing)
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
        const float tmj = quad_bcast<B>(tms[k]), tyj = quad_bcast<B>(tys[k]);                                                  \
        color.x = fmaf(trj * cxj, ae, color.x);                                                                                \
        color.y = fmaf(trj * cyj, ae, color.y);                                                                                \
        color.z = fmaf(trj * czj, ae, color.z);                                                                                \
        S = fmaf(trj * tmj, ae, S);                                                                                            \
        alpha = fmaf(trj, ae, alpha);                                                                                          \
        ray_steps += live ? 1u : 0u;                                                                                           \
        const bool cross = !reached && ae > 0.f && alpha >= tau;                                                               \
        d = cross ? tyj : d;                                                                                                   \
        kc = cross ? ray_steps : kc;                                                                                           \
        reached = reached || cross;                                                                                            \
      }
      OVR_STEP(0) OVR_STEP(1) OVR_STEP(2) OVR_STEP(3)
#undef OVR_STEP
      const bool mlive = sub == 0 ? lv[0] : sub == 1 ? lv[1] : sub == 2 ? lv[2] : lv[3];
      n_samples += mlive ? 1u : 0u;
      n_shaded += (mlive && aa[k] > 0.f) ? 1u : 0u;
      t_exit = mlive ? tys[k] : t_exit;
    }
  }
  DepthOutputResult r;
  {
    const float s = __uint_as_float(n_shaded);
    r.opaque = __float_as_uint(quad_bcast<0>(s)) + __float_as_uint(quad_bcast<1>(s)) + __float_as_uint(quad_bcast<2>(s)) + __float_as_uint(quad_bcast<3>(s));
    r.tx = fmaxf(fmaxf(quad_bcast<0>(t_exit), quad_bcast<1>(t_exit)), fmaxf(quad_bcast<2>(t_exit), quad_bcast<3>(t_exit))); // (ty only grows along a ray)
  }
  r.steps = ray_steps;
  r.alpha = alpha;
  r.color = color;
  r.S = S;
  r.d = d;
  r.k = kc;
  r.reached = reached;
  r.fetched = n_samples;
  r.shaded = n_shaded;
  return r;
}

// a depth frame: the depth-limited kernel's frame around depth_output_ray; the pixel is the march's un-premultiplied one, the layer the sum over the pixel's
// samples of (d if reached else 0, S, 1 if reached else 0), scaled by 1 / spp like every layer.  LDS: [axis tables][TF colour][TF alpha].  P.max_depth, where
// it is not null, holds P.width x P.height values (the host binds it only then); without an image z = +inf takes no load
template <int VT, int AM, int SHADE, bool ORTHO = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, kMarchWavesPerEu))) void depth_output_kernel(const RayMarchParams P)
{
  static_assert(depth_output_variant_exists(SHADE, AM, false, true, ORTHO) && (AM != 4 || RowLoads<VT, 4>::on), "no such variant of the depth-output kernel (host/launch_plan.hpp)");
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
  const float z = (active && P.max_depth) ? P.max_depth[pixel_index] : __builtin_inff(); // the pixel's: every sample takes it
  const float tau = P.depth_tau;
  unsigned int v0 = (unsigned int)P.frame_index, v1 = pixel_index; // RandomTEA(frame_index, pixel_index)
  float o_a = 0.f;
  f3 o_c = mk3(0, 0, 0), o_l = mk3(0, 0, 0);
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
    const DepthOutputResult mr = depth_output_ray<VT, AM, SHADE, ORTHO>(P, vc, tf, mc, org, dir, t0, max_depth_cut(t1, z), live, tau, subm);
    n_samples += mr.fetched;
    n_shaded += mr.shaded;
    // the march's pixel sample: alpha_blend with an always-missing background
    o_a += mr.alpha;
    if (mr.alpha > 0.f) { o_c.x += mr.color.x / mr.alpha; o_c.y += mr.color.y / mr.alpha; o_c.z += mr.color.z / mr.alpha; }
    // the depth layer's: (d, S, reached) - d is 0 while not reached
    o_l.x += mr.d;
    o_l.y += mr.S;
    o_l.z += mr.reached ? 1.f : 0.f;
  }
  if (active && owner) {
    const float rspp = 1.f / (float)P.spp;
    o_a *= rspp;
    o_c.x *= rspp; o_c.y *= rspp; o_c.z *= rspp;
    o_l.x *= rspp; o_l.y *= rspp; o_l.z *= rspp;
    write_pixel(P, pixel_index, o_c, o_a, o_l);
  }
  store_block_counters(P, reinterpret_cast<unsigned int*>(lds_raw), lane, wave, n_rays, n_samples, n_shaded, 0u, (active && owner) ? 1u : 0u, 0u, 0u, n_outside_hits);
}

// the known-answer entry's kernel: ray i = the quad of lanes 4 i ... 4 i + 3, ending on depth[i] (depth == nullptr: no limit on any ray), through
// depth_output_ray as the frame's kernel calls it (the perspective camera's view vector: the rays are the caller's).  out, 12 floats per ray: the depth limit's
// eight (steps taken, the cut tc, tx at exit, steps with a > 0, r, g, b, a of the pixel sample), then reached, d, k, S
template <int VT, int AM, int SHADE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, kMarchWavesPerEu))) void depth_output_floats_kernel(const RayMarchParams P, const float* org, const float* dir, const float* depth, float* out, long long n)
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
  const float tc = max_depth_cut(t1, depth ? depth[j] : __builtin_inff());
  const DepthOutputResult mr = depth_output_ray<VT, AM, SHADE, false>(P, vc, tf, mc, o, d, t0, tc, live, P.depth_tau, subm);
  if (valid && sub == 0) {
    const bool lit = mr.alpha > 0.f;
    float* q = out + 12 * i;
    q[0] = (float)mr.steps; q[1] = live ? tc : 0.f; q[2] = live ? mr.tx : 0.f; q[3] = (float)mr.opaque;
    q[4] = lit ? mr.color.x / mr.alpha : 0.f; q[5] = lit ? mr.color.y / mr.alpha : 0.f; q[6] = lit ? mr.color.z / mr.alpha : 0.f; q[7] = mr.alpha;
    q[8] = mr.reached ? 1.f : 0.f; q[9] = mr.d; q[10] = (float)mr.k; q[11] = mr.S;
  }
}

struct DepthOutputKernels { FrameKernel frame = nullptr; MaxDepthFloatsKernel floats = nullptr; }; // nullptr: no such variant of this type
// the variants: bit 0 the camera kind, bit 1 the shading mode
template <int VT, int AM> struct DepthOutputVariants {
  template <unsigned I> static constexpr DepthOutputKernels at()
  {
    if constexpr (!depth_output_variant_exists((I >> 1) & 1, AM, false, true, (I & 1u) != 0)) return {};
    else return { depth_output_kernel<VT, AM, (I >> 1) & 1, (I & 1u) != 0>, depth_output_floats_kernel<VT, AM, (I >> 1) & 1> };
  }
};
// a depth-output plan's kernels of a voxel type; nullptr for a replica's type (or mode 4 on a layout without row loads), like max_depth_kernels_of
template <int VT>
DepthOutputKernels depth_output_kernels_of(const LaunchPlan& pl)
{
  if (pl.error || !pl.depth_output.on || !pl.depth_output.clipped || pl.skip) return DepthOutputKernels();
  const unsigned i = (pl.orthographic ? 1u : 0u) | (pl.depth_output.shade ? 2u : 0u);
  return dispatch_addressing<DepthOutputKernels, VT, true>(pl.am, [&](auto m) { return variant_at<DepthOutputVariants<VT, decltype(m)::value>>(i, std::make_integer_sequence<unsigned, 4>()); });
}

} // namespace ovrhip
