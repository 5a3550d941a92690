// ovr_hip_preintegration.h - pre-integrated classification (include/ovr_hip.h ovr_hip_set_preintegration; open-volume-renderer_amd/preintegration.py is the
// normative arithmetic): the unshaded march in which every SEGMENT between two consecutive samples is classified by the integral of the
// transfer function over the values the segment spans, read from a node table of cumulative integrals (host/preintegration_host.hpp builds it).  Nothing is
// restated that exists: the tap, the transfer function in LDS (stage_tf, tf_coord, tf_alpha, tf_color), the opacity correction and the quad helpers are
// ovr_hip_device.h's, called as raymarch_kernel calls them; the frame shell is the slice context kernel's.
//
// One kernel, preintegrated_kernel<VT, AM, ORTHO>, in the in-place march's place in the launch sequence; it exists with the clipped box test alone (a frame
// without a clip box runs it with the unit box, whose bounds give the unclipped test's bits - DESIGN.md section 12), for both cameras.  Four lanes per ray; a
// round is kProjectK x 4 segments.  Lane `sub` owns segments 4 k + sub and taps at its segment's BACK end; the front value of a segment is the back value of
// the segment before it and comes from the neighbouring lane by a DPP quad permute - for sub == 0 from lane 3 of the previous k, carried across rounds.  The
// ray's entry tap rides with the first round's gathers.  So there is one gather group per segment plus one per ray and one node lookup (two adjacent 128-bit
// LDS reads) per segment: the (T, K) pair of an endpoint travels with its value.  The alpha / colour recurrence, the loop condition tested before every
// segment and the transparent-round shortcut are the slice context kernel's.
// The two classifications - the march's own at the mean coordinate while the endpoints lie less than a node apart, the integral otherwise - are computed under
// wave-uniform branches (a wave whose segments all take one of them skips the other) and selected per lane.  A segment whose opacity is 0 in every lane of the
// wave's step is not coloured.  With every voxel equal every segment takes the first branch at um = uf: the frame is raymarch_kernel<VT, 0, AM>'s bit for bit.
// The product evaluates exp2 with v_exp_f32 and both divisions as IEEE divides (reciprocal multiplies were not tried); the exact-parity build det_exp2f.
#pragma once

#include "ovr_hip_slices.h" // (the frame shell: slice_sample_position)

namespace ovrhip {

struct PreintConsts {
  const float4* nodes; // LDS: M + 1 nodes (T, Kr, Kg, Kb), 16-byte aligned
  float fm1;           // (float)(M - 1)
};

// lane sub's value of lane sub - 1 of its quad (lane 0 keeps its own: the caller replaces it)
__device__ __forceinline__ float quad_prev(float x)
{
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x90, 0xf, 0xf, true)); // quad_perm [0, 0, 1, 2]
}
__device__ __forceinline__ float4 quad_prev4(float4 v) { return make_float4(quad_prev(v.x), quad_prev(v.y), quad_prev(v.z), quad_prev(v.w)); }
template <int B> __device__ __forceinline__ float4 quad_bcast4(float4 v) { return make_float4(quad_bcast<B>(v.x), quad_bcast<B>(v.y), quad_bcast<B>(v.z), quad_bcast<B>(v.w)); }

// the node lerp at u in [0, 1]: i0 = (int)(u * (M - 1)), the fraction, the lerp of nodes i0 and i0 + 1 (the table's last entry is a copy: no min)
__device__ __forceinline__ float4 preint_lookup(const PreintConsts& pc, float u)
{
  const float x = u * pc.fm1;
  const int i0 = (int)x;
  const float f = __builtin_amdgcn_fractf(x);
  const float4 a = pc.nodes[i0], b = pc.nodes[i0 + 1];
  return make_float4(lerpf(a.x, b.x, f), lerpf(a.y, b.y, f), lerpf(a.z, b.z, f), lerpf(a.w, b.w, f));
}
__device__ __forceinline__ float preint_exp2(float x)
{
#if OVR_PARITY_EXACT
  return det_exp2f(x);
#else
  return __builtin_amdgcn_exp2f(x);
#endif
}

struct PreintResult {         // quad-uniform but for the two counters
  unsigned int steps;         // segments taken (the ray's; the entry tap is not a segment)
  unsigned int integral;      // of them, segments classified by the integral branch
  float tx;                   // tx at exit: the back end of the last segment taken, t0 without one
  float alpha;
  f3 color;                   // premultiplied
  unsigned int fetched, shaded; // THIS LANE's: segments taken; segments with a > 0
};

template <int VT, int AM>
__device__ __forceinline__ PreintResult preintegrated_ray(const VolConsts& vc, const TfConsts& tf, const PreintConsts& pc, const MarchConsts& mc, f3 org, f3 dir,
                                                          float t0, float t1, bool hit, const SubMask& subm)
{
  constexpr int K = kProjectK;
  const int sub = subm.sub;
  float alpha = 0.f;
  f3 color = mk3(0, 0, 0);
  unsigned int n_samples = 0, n_shaded = 0, n_integral = 0;
  bool live = hit;
  bool first = true; // wave-uniform: every ray of the wave starts with the loop
  float tx = t0, ty = fminf(t1, t0 + mc.step);
  float t_exit = t0;
  float carry_u = 0.f;                        // the back value of the last segment of the round before (first round: the entry tap's)
  float4 carry_n = make_float4(0, 0, 0, 0);   // and its node lerp
  while (__ballot(live) != 0ull) {
    // the ray's next 4K segments: every lane runs the (tx, ty) recurrence, keeps its own K segments and one validity bit per segment
    unsigned int vmask = 0;
    Tap taps[K];
    float dts[K], tys[K];
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
      tys[k] = mty;
    }
    Tap tap_e;
    if (first) { // the entry tap, at t0: issued with the round's gathers
      const f3 pos = mk3(fmaf(t0, dir.x, org.x), fmaf(t0, dir.y, org.y), fmaf(t0, dir.z, org.z));
      tap_coords(vc, to_object(mc, pos), tap_e);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) { // ONE tap per segment, at its back end
      const f3 pos = mk3(fmaf(tys[k], dir.x, org.x), fmaf(tys[k], dir.y, org.y), fmaf(tys[k], dir.z, org.z));
      tap_coords(vc, to_object(mc, pos), taps[k]);
    }
    // branch-free, like the march: dead lanes load (their coordinates are clamped, the loads are in bounds) and feed a = 0
    if (first) tap_loads<VT, AM>(vc, tap_e);
#pragma unroll
    for (int k = 0; k < K; ++k) tap_loads<VT, AM>(vc, taps[k]);
    if (first) {
      carry_u = tf_coord(tf, tap_finish<VT>(vc, tap_e));
      carry_n = preint_lookup(pc, carry_u);
      first = false;
    }
    // own segments: the back value and its node lerp, the front pair from the neighbour, the classification
    float aa[K];
    f3 ca[K];
    unsigned int imask = 0; // own segments on the integral branch
    {
      float prev_u = carry_u;
      float4 prev_n = carry_n;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float ub = tf_coord(tf, tap_finish<VT>(vc, taps[k]));
        const float4 nb = preint_lookup(pc, ub);
        const float qu = quad_prev(ub);
        const float4 qn = quad_prev4(nb);
        const bool head = sub == 0;
        const float uf = head ? prev_u : qu;
        const float4 nf = head ? prev_n : qn;
        prev_u = quad_bcast<3>(ub);
        prev_n = quad_bcast4<3>(nb);
        const float du = ub - uf, adj = mc.base * dts[k];
        const bool first_branch = fabsf(du) * pc.fm1 < 1.f; // less than a node apart: the march's own classification
        const float um = 0.5f * (uf + ub);
        float a1 = 0.f, a2 = 0.f;
        if (__ballot(first_branch) != 0ull) a1 = opacity_correction<false>(tf_alpha<true>(tf, um), adj);
        float td = 0.f;
        if (__ballot(!first_branch) != 0ull) {
          td = nb.x - nf.x;
          a2 = clamp01(1.f - preint_exp2(-((td / du) * adj)));
        }
        aa[k] = first_branch ? a1 : a2;
        imask |= first_branch ? 0u : (1u << k);
        // the colour: only where a lane of the wave's step has opacity (a = 0 adds exactly 0 whatever the colour)
        f3 c = mk3(0, 0, 0);
        if (__ballot(aa[k] > 0.f && live) != 0ull) {
          f3 c1 = mk3(0, 0, 0), c2 = mk3(0, 0, 0);
          if (__ballot(first_branch) != 0ull) {
            const f3 rgb = tf_color(tf, um);
            c1 = mk3(clamp01(rgb.x), clamp01(rgb.y), clamp01(rgb.z));
          }
          if (__ballot(!first_branch) != 0ull) {
            const bool some = td != 0.f;
            c2 = mk3(some ? clamp01((nb.y - nf.y) / td) : 0.f, some ? clamp01((nb.z - nf.z) / td) : 0.f, some ? clamp01((nb.w - nf.w) / td) : 0.f);
          }
          c = first_branch ? c1 : c2;
        }
        ca[k] = c;
      }
      carry_u = prev_u;
      carry_n = prev_n;
    }
    // transparent round (wave-uniform): no live segment of any ray of the wave has opacity > 0 - every segment adds exactly 0; only liveness and the counters move
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
          n_integral += (mlive && ((imask >> k) & 1u) != 0u) ? 1u : 0u;
          t_exit = mlive ? tys[k] : t_exit;
        }
        live = go && ((vmask >> (4 * K - 1)) & 1u) != 0u;
        continue;
      }
    }
    // the ray's recurrence over the 4K segments, in order; every lane of the quad computes all of it (a dead segment feeds a = 0: fma(tr, 0, x) == x exactly)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      bool lv[4]; // the loop condition at each segment
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
      n_integral += (mlive && ((imask >> k) & 1u) != 0u) ? 1u : 0u;
      t_exit = mlive ? tys[k] : t_exit;
    }
  }
  PreintResult r;
  {
    const float o = __uint_as_float(n_samples), i = __uint_as_float(n_integral);
    r.steps = __float_as_uint(quad_bcast<0>(o)) + __float_as_uint(quad_bcast<1>(o)) + __float_as_uint(quad_bcast<2>(o)) + __float_as_uint(quad_bcast<3>(o));
    r.integral = __float_as_uint(quad_bcast<0>(i)) + __float_as_uint(quad_bcast<1>(i)) + __float_as_uint(quad_bcast<2>(i)) + __float_as_uint(quad_bcast<3>(i));
    r.tx = fmaxf(fmaxf(quad_bcast<0>(t_exit), quad_bcast<1>(t_exit)), fmaxf(quad_bcast<2>(t_exit), quad_bcast<3>(t_exit))); // (ty only grows along a ray)
  }
  r.alpha = alpha;
  r.color = color;
  r.fetched = n_samples;
  r.shaded = n_shaded;
  return r;
}

// LDS: [axis tables][TF colour][TF alpha][node table, 16-byte aligned] (plan_preintegrated sizes it)
template <int VT, int AM>
__device__ __forceinline__ void preintegrated_stage(const RayMarchParams& P, unsigned char* lds_raw, VolConsts& vc, TfConsts& tf, PreintConsts& pc)
{
  const size_t tb = (stage_tables<VT, AM>(P, lds_raw, vc) + 15) & ~(size_t)15;
  const size_t nb = align16(tb + tf_lds_bytes(P.n_color, P.n_alpha));
  float4* ln = reinterpret_cast<float4*>(lds_raw + nb);
  const float4* gn = reinterpret_cast<const float4*>(P.preint_nodes);
  for (int i = threadIdx.x; i <= P.preint_m1 + 1; i += kBlock) ln[i] = gn[i]; // M + 1 entries: the host's table carries the copy of the last
  pc.nodes = ln;
  pc.fm1 = (float)P.preint_m1;
  stage_tf(P, lds_raw + tb, true, tf); // (ends on a barrier)
}

// a pre-integrated frame: the slice context kernel's frame around preintegrated_ray; the pixel is the march's un-premultiplied one, the gradient layer zero.
// The register budget is the march's: at most 3 waves per SIMD
template <int VT, int AM, bool ORTHO = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, kMarchWavesPerEu))) void preintegrated_kernel(const RayMarchParams P)
{
  static_assert(preintegrated_variant_exists(AM, false, true, ORTHO) && (AM != 4 || RowLoads<VT, 4>::on), "no such variant of the pre-integrated kernel (host/launch_plan.hpp)");
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
  PreintConsts pc;
  const bool staged = __syncthreads_or(active ? 1 : 0) != 0; // workgroup-uniform
  if (staged) preintegrated_stage<VT, AM>(P, lds_raw, vc, tf, pc);
  else {
    tf = TfConsts{};
    pc = PreintConsts{};
    vc.tab_x = vc.tab_y = vc.tab_z = nullptr;
    vc.tab_z64 = nullptr;
  }
  unsigned int n_rays = 0, n_samples = 0, n_shaded = 0, n_outside_hits = 0;
  const float rsx = 1.f / (float)P.width, rsy = 1.f / (float)P.height;
  const float scx = ((float)ix + .5f) * rsx, scy = ((float)iy + .5f) * rsy;
  const unsigned int pixel_index = (unsigned int)ix + (unsigned int)iy * (unsigned int)P.width;
  unsigned int v0 = (unsigned int)P.frame_index, v1 = pixel_index; // RandomTEA(frame_index, pixel_index)
  float o_a = 0.f;
  f3 o_c = mk3(0, 0, 0);
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
    const PreintResult pr = preintegrated_ray<VT, AM>(vc, tf, pc, mc, org, dir, t0, t1, live, subm);
    n_samples += pr.fetched;
    n_shaded += pr.shaded;
    // the march's pixel sample: alpha_blend with an always-missing background
    o_a += pr.alpha;
    if (pr.alpha > 0.f) { o_c.x += pr.color.x / pr.alpha; o_c.y += pr.color.y / pr.alpha; o_c.z += pr.color.z / pr.alpha; }
  }
  if (active && owner) {
    const float rspp = 1.f / (float)P.spp;
    o_a *= rspp;
    o_c.x *= rspp; o_c.y *= rspp; o_c.z *= rspp;
    write_pixel(P, pixel_index, o_c, o_a, mk3(0, 0, 0));
  }
  store_block_counters(P, reinterpret_cast<unsigned int*>(lds_raw), lane, wave, n_rays, n_samples, n_shaded, 0u, (active && owner) ? 1u : 0u, 0u, 0u, n_outside_hits);
}

// the known-answer entry's kernel: ray i = the quad of lanes 4 i ... 4 i + 3, through preintegrated_ray as the frame's kernel calls it.
// out: (segments taken, of them integral-branch segments, tx at exit, 0, r, g, b, a of the pixel sample) per ray
template <int VT, int AM>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, kMarchWavesPerEu))) void preintegrated_floats_kernel(const RayMarchParams P, const float* org, const float* dir, float* out, long long n)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int sub = threadIdx.x & 3;
  const SubMask subm = make_submask(sub);
  VolConsts vc;
  MarchConsts mc;
  setup_consts(P, vc, mc);
  TfConsts tf;
  PreintConsts pc;
  preintegrated_stage<VT, AM>(P, lds_raw, vc, tf, pc);
  const long long i = ((long long)blockIdx.x * kBlock + threadIdx.x) >> 2;
  const bool valid = i < n;
  const long long j = valid ? i : 0;
  const f3 o = mk3(org[3 * j], org[3 * j + 1], org[3 * j + 2]), d = mk3(dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]);
  const f3 oo = to_object(mc, o), od = mk3(d.x * mc.inv_scale.x, d.y * mc.inv_scale.y, d.z * mc.inv_scale.z);
  float t0 = 0.f, t1 = FLT_MAX;
  const bool live = valid && box_test<true>(P, t0, t1, oo, od);
  const PreintResult pr = preintegrated_ray<VT, AM>(vc, tf, pc, mc, o, d, t0, t1, live, subm);
  if (valid && sub == 0) {
    const bool lit = pr.alpha > 0.f;
    float* q = out + 8 * i;
    q[0] = (float)pr.steps; q[1] = (float)pr.integral; q[2] = live ? pr.tx : 0.f; q[3] = 0.f;
    q[4] = lit ? pr.color.x / pr.alpha : 0.f; q[5] = lit ? pr.color.y / pr.alpha : 0.f; q[6] = lit ? pr.color.z / pr.alpha : 0.f; q[7] = pr.alpha;
  }
}

typedef void (*PreintegratedFloatsKernel)(const RayMarchParams, const float*, const float*, float*, long long);
struct PreintegratedKernels { FrameKernel frame = nullptr; PreintegratedFloatsKernel floats = nullptr; }; // nullptr: no such variant of this type
// the variants: the camera kind alone
template <int VT, int AM> struct PreintegratedVariants {
  template <unsigned I> static constexpr PreintegratedKernels at()
  {
    if constexpr (!preintegrated_variant_exists(AM, false, true, I != 0)) return {};
    else return { preintegrated_kernel<VT, AM, I != 0>, preintegrated_floats_kernel<VT, AM> };
  }
};
// a pre-integrated plan's kernels of a voxel type; nullptr for a replica's type (or mode 4 on a layout without row loads), like slice_context_kernels_of
template <int VT>
PreintegratedKernels preintegrated_kernels_of(const LaunchPlan& pl)
{
  if (pl.error || !pl.preintegrated.on || !pl.preintegrated.clipped || pl.skip) return PreintegratedKernels();
  const unsigned i = pl.orthographic ? 1u : 0u;
  return dispatch_addressing<PreintegratedKernels, VT, true>(pl.am, [&](auto m) { return variant_at<PreintegratedVariants<VT, decltype(m)::value>>(i, std::make_integer_sequence<unsigned, 2>()); });
}

} // namespace ovrhip
