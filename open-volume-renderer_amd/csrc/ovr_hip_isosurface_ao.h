// ovr_hip_isosurface_ao.h - ambient occlusion of the isosurface frames (include/ovr_hip.h ovr_hip_set_ambient_occlusion; DESIGN.md section 20;
// open-volume-renderer_amd/isosurface.py is the arithmetic): K occlusion walks over the hemisphere of every event, cut at a radius, scale the event's ambient
// coefficient.  The AO kernels are twins of the TRANSLUCENT ones (an opaque frame runs them with its all-ones opacities: section 19's identity) and live in an
// object of their own per type (ovr_hip_isosurface.hip with -DOVR_ISO_AO): ovr_hip_device.h is what it was, and what the twins share with isosurface_layers - the
// loop over walks and events - is restated here, as section 19 restated the refinement.
#pragma once
#include "ovr_hip_device.h"

namespace ovrhip {

constexpr int kAoMaxSamples = 16, kAoRotations = 16; // include/ovr_hip.h OVR_HIP_MAX_AO_SAMPLES / OVR_HIP_AO_ROTATIONS

// what the AO walks of one event found
struct IsoAo {
  float O;                                  // the occlusion (quad-uniform, like steps): the mean of the K walks' accumulated opacities
  unsigned int steps;                       // the steps of the K walks
  unsigned int fetched, skipped;            // THIS LANE's
};

// the K occlusion walks of the event at pos with the world normal n_w, seen along dir; m: the rotation of the direction table (quad-uniform, 0 ... 15).
// Each walk is iso_point's shadow walk with d_j in the light's place, its far end cut at P.ao_distance: four steps of one ray per quad instruction.  Every loop
// is bounded: K <= 16 passes, and a pass of a ray that goes on has consumed at least one of its steps.  hit: the quad has the event (the others tap along:
// every position goes through tap_coords, which clamps it, so every load is in bounds)
template <int VT, int AM, bool SKIP, bool CLIP>
__device__ __forceinline__ IsoAo iso_ao(const RayMarchParams& P, const VolConsts& vc, const MarchConsts& mc, f3 pos, f3 n_w, f3 dir, int m, bool hit, const SubMask& subm)
{
  IsoAo r;
  r.O = 0.f; r.steps = 0u; r.fetched = r.skipped = 0u;
  // the normal that faces the viewer (a NaN normal stays NaN: its rays miss the box)
  const bool front = dot3(n_w, dir) <= 0.f;
  const f3 N = front ? n_w : mk3(-n_w.x, -n_w.y, -n_w.z);
  // Duff et al.'s branch-free orthonormal basis around N, every operation on its own
  const float sg = copysignf(1.f, N.z);
  const float a = -1.f / (sg + N.z);
  const float b = (N.x * N.y) * a;
  const f3 T = mk3(1.f + ((sg * N.x) * N.x) * a, sg * b, -(sg * N.x));
  const f3 B = mk3(b, sg + (N.y * N.y) * a, -N.y);
  const f3 oo = to_object(mc, pos);
  const int K = P.ao_samples;
  const float* tab = P.ao_dirs + 3 * (m * K);
  float S = 0.f;
#pragma unroll 1
  for (int j = 0; j < K; ++j) {
    const float lx = tab[3 * j], ly = tab[3 * j + 1], lz = tab[3 * j + 2];
    const f3 d = mk3(fmaf(lx, T.x, fmaf(ly, B.x, lz * N.x)), fmaf(lx, T.y, fmaf(ly, B.y, lz * N.y)), fmaf(lx, T.z, fmaf(ly, B.z, lz * N.z)));
    const f3 od = mk3(d.x * mc.inv_scale.x, d.y * mc.inv_scale.y, d.z * mc.inv_scale.z);
    float a0 = 0.f, a1 = FLT_MAX;
    bool go = box_test<CLIP>(P, a0, a1, oo, od) && hit;
    a1 = fminf(a1, P.ao_distance);
    IsoCarry sc;
    sc.side = -1; sc.tm = 0.f; sc.ty = 0.f;
    float Aj = 0.f, stx = a0 + mc.step;
    while (__ballot(go) != 0ull) {
      const IsoWalk sw = iso_walk<VT, AM, SKIP, true>(P, vc, mc, pos, d, stx, a1, go, subm, &sc);
      r.fetched += sw.fetched; r.skipped += sw.skipped; r.steps += sw.steps;
      if (sw.hit) {
        int k, dk, n;
        iso_step_events(sw.side_a, sw.side_b, k, dk, n);
#pragma unroll
        for (int e = 0; e < kMaxIsovalues; ++e) {
          if (e < n && !(Aj >= 0.9999f)) Aj = fmaf(1.f - Aj, iso_opacity(P, k), Aj);
          k += dk;
        }
      }
      go = sw.hit && !(Aj >= 0.9999f);
      stx = sc.ty; sc.side = sw.side_b; sc.tm = sw.tb;
    }
    S += Aj;
  }
  r.O = S / (float)K;
  return r;
}

// a translucent ray with ambient occlusion: isosurface_layers (ovr_hip_device.h) with iso_ao behind every event's iso_point, in the same wave-uniform branch.
// rot0: the rotation index of the ray's sample.  on_event(index, k, iso, alpha, tr, A after, point, O).  `ao` receives the AO walks' steps (quad-uniform)
// and THIS LANE's fetched / skipped counts
template <int VT, int AM, int SHADE, bool SKIP, bool CLIP, class OnEvent>
__device__ __forceinline__ IsoLayers isosurface_layers_ao(const RayMarchParams& P, const VolConsts& vc, const MarchConsts& mc, f3 org, f3 dir, float t0, float t1, bool live,
                                                          int rot0, const SubMask& subm, IsoAo& ao, OnEvent&& on_event)
{
  static_assert(isosurface_variant_exists(SHADE, AM, SKIP, CLIP, false, true, true), "no such variant of the isosurface kernel (host/launch_plan.hpp)");
  IsoLayers L;
  L.events = 0u; L.A = 0.f; L.iso = L.t = 0.f; L.steps = L.shadow_steps = 0u; L.fetched = L.skipped = L.shadow_fetched = L.shadow_skipped = 0u;
  ao.O = 0.f; ao.steps = 0u; ao.fetched = ao.skipped = 0u;
  IsoCarry carry;
  carry.side = -1; carry.tm = 0.f; carry.ty = t0;
  float tx = t0;
  bool go = live;
  while (__ballot(go) != 0ull) {
    const IsoWalk w = iso_walk<VT, AM, SKIP, true>(P, vc, mc, org, dir, tx, t1, go, subm, &carry);
    L.steps += w.steps; L.fetched += w.fetched; L.skipped += w.skipped;
    int k = 0, dk = 0, n = 0;
    if (w.hit) iso_step_events(w.side_a, w.side_b, k, dk, n);
    bool open = w.hit; // the ray takes the step's next event
#pragma unroll 1
    for (int e = 0; e < kMaxIsovalues; ++e) {
      const bool ev = open && e < n;
      if (__ballot(ev) == 0ull) break; // (wave-uniform: the quad exchanges of iso_point and iso_ao run with every lane)
      const float iso = iso_value(P, k), alpha = iso_opacity(P, k);
      IsoPoint pt;
      pt.t = 0.f; pt.pos = org; pt.n_w = mk3(0, 0, 0); pt.shadow = 0.f; pt.shadow_steps = pt.shadow_fetched = pt.shadow_skipped = 0u;
      iso_point<VT, AM, SHADE, SKIP, CLIP>(P, vc, mc, org, dir, iso, w.ta, w.tb, ev, subm, pt);
      L.shadow_fetched += pt.shadow_fetched; L.shadow_skipped += pt.shadow_skipped; // (a quad without the event walked no shadow step)
      const IsoAo o = iso_ao<VT, AM, SKIP, CLIP>(P, vc, mc, pt.pos, pt.n_w, dir, rot0, ev, subm);
      ao.fetched += o.fetched; ao.skipped += o.skipped; // (nor an AO step)
      if (ev) {
        const float tr = 1.f - L.A;
        const float A = fmaf(tr, alpha, L.A);
        on_event(L.events, k, iso, alpha, tr, A, pt, o.O);
        if (L.events == 0u) { L.iso = iso; L.t = pt.t; }
        L.A = A;
        ++L.events;
        L.shadow_steps += pt.shadow_steps;
        ao.steps += o.steps;
        open = !(A >= 0.9999f);
      }
      k += dk;
    }
    go = w.hit && open;
    tx = carry.ty; carry.side = w.side_b; carry.tm = w.tb;
  }
  return L;
}

// the rotation of the direction table for sample k_spp of the frame at pixel (ix, iy): interleaved over 4 x 4 pixels, advancing with every accumulated sample
__device__ __forceinline__ int ao_rotation(const RayMarchParams& P, int ix, int iy, int k_spp)
{
  return ((ix & 3) + 4 * (iy & 3) + (P.frame_index - 1) * P.spp + k_spp) & (kAoRotations - 1);
}

// an isosurface frame with ambient occlusion: isosurface_kernel's TRANS frame (ovr_hip_device.h) around isosurface_layers_ao; the event's shade factor takes
// ka * (1 - O) for the ambient coefficient.  The AO walks' fetched / dropped steps count with the shadow walks'
template <int VT, int AM, int SHADE, bool SKIP, bool ORTHO>
__global__ __launch_bounds__(kBlock) void isosurface_ao_kernel(const RayMarchParams P)
{
  static_assert(isosurface_variant_exists(SHADE, AM, SKIP, true, ORTHO, true, true) && (AM != 4 || RowLoads<VT, 4>::on), "no such variant of the isosurface kernel (host/launch_plan.hpp)");
  constexpr bool CLIP = true;
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
  const bool any_active = __syncthreads_or(active ? 1 : 0) != 0;
  if (any_active) {
    stage_tables<VT, AM>(P, lds_raw, vc);
    __syncthreads();
  }
  else {
    vc.tab_x = vc.tab_y = vc.tab_z = nullptr;
    vc.tab_z64 = nullptr;
  }
  unsigned int n_rays = 0, n_samples = 0, n_skipped = 0, n_hits = 0, n_shadow = 0, n_shadow_skipped = 0, n_outside_hits = 0;
  const float rsx = 1.f / (float)P.width, rsy = 1.f / (float)P.height;
  const float scx = ((float)ix + .5f) * rsx, scy = ((float)iy + .5f) * rsy;
  const unsigned int pixel_index = (unsigned int)ix + (unsigned int)iy * (unsigned int)P.width;
  unsigned int v0 = (unsigned int)P.frame_index, v1 = pixel_index; // RandomTEA(frame_index, pixel_index)
  float o_a = 0.f;
  f3 o_c = mk3(0, 0, 0), o_g = mk3(0, 0, 0);
  for (int k_spp = 0; any_active && k_spp < P.spp; ++k_spp) { // uniform trip count (a workgroup without a pixel has no tables: it taps nothing)
    float sx = scx, sy = scy;
    if (P.jitter_mode == 1) {
      float j0, j1;
      jitter_global(P, ix, iy, k_spp, j0, j1);
      sx += (j0 - 0.5f) * rsx;
      sy += (j1 - 0.5f) * rsy;
    }
    else if (P.spp > 1) {
      tea16(v0, v1);
      sx += ((float)v0 * OVR_TEA_TOFLOAT - 0.5f) * rsx;
      sy += ((float)v1 * OVR_TEA_TOFLOAT - 0.5f) * rsy;
    }
    const float ux = sx - 0.5f, uy = sy - 0.5f;
    f3 org, dir;
    pixel_ray<ORTHO>(P, ux, uy, org, dir);
    const f3 oo = to_object(mc, org);
    const f3 od = mk3(dir.x * mc.inv_scale.x, dir.y * mc.inv_scale.y, dir.z * mc.inv_scale.z);
    float t0 = 0.f, t1 = FLT_MAX;
    const bool live = active && primary_box_test<CLIP, ORTHO>(P, t0, t1, oo, od);
    if (active && owner) ++n_rays;
    if (live && owner && box_ignored_slab_outside<CLIP>(P, oo, od)) ++n_outside_hits;
    // the colour lookup and the shade factor in front of the composite: C_ch = fma(tr * c_ch, alpha, C_ch), the march's expression
    f3 cc = mk3(0, 0, 0);
    auto on_event = [&](unsigned int, int, float iso, float alpha, float tr, float, const IsoPoint& pt, float O) {
      if (!owner) return;
      f3 c = isosurface_colour(P, iso);
      const float lit = shade_light<true, ORTHO>(P, mc.light, pt.n_w, pt.pos);
      const float shade = P.mat_ka * (1.f - O) + lit * (1.f - pt.shadow); // shade_factor with ambient = ka (1 - O)
      c = mk3(clamp01(c.x * shade), clamp01(c.y * shade), clamp01(c.z * shade));
      cc.x = fmaf(tr * c.x, alpha, cc.x); cc.y = fmaf(tr * c.y, alpha, cc.y); cc.z = fmaf(tr * c.z, alpha, cc.z);
    };
    IsoAo ao;
    const IsoLayers il = isosurface_layers_ao<VT, AM, SHADE, SKIP, CLIP>(P, vc, mc, org, dir, t0, t1, live, ao_rotation(P, ix, iy, k_spp), subm, ao, on_event);
    n_samples += il.fetched;
    n_skipped += il.skipped;
    n_shadow += il.shadow_fetched + ao.fetched;
    n_shadow_skipped += il.shadow_skipped + ao.skipped;
    if (il.events > 0u && owner) {
      n_hits += il.events;
      o_c.x += cc.x / il.A; o_c.y += cc.y / il.A; o_c.z += cc.z / il.A;
      o_a += il.A;
      o_g.x += il.iso; o_g.y += il.t; o_g.z += 1.f;
    }
  }
  if (active && owner) {
    const float rspp = 1.f / (float)P.spp;
    o_a *= rspp;
    o_c.x *= rspp; o_c.y *= rspp; o_c.z *= rspp;
    o_g.x *= rspp; o_g.y *= rspp; o_g.z *= rspp;
    write_pixel(P, pixel_index, o_c, o_a, o_g);
  }
  store_block_counters(P, reinterpret_cast<unsigned int*>(lds_raw), lane, wave, n_rays, n_samples, n_hits, n_shadow, (active && owner) ? 1u : 0u, n_skipped, n_shadow_skipped,
                       n_outside_hits);
}

// the known-answer entry's kernel (ovr_hip_isosurface_ao_floats): ray i = the quad of lanes 4 i ... 4 i + 3 through isosurface_layers_ao as the frame's kernel calls
// it with full shading and the rotation `rotation` -> 8 + 8 max_events floats: (events composited, A, steps walked, shadow steps over all events, the AO walks'
// steps, the AO walks' fetched steps, 0, 0), then per event e < min(events, max_events) (k, t*, n_w.x, n_w.y, n_w.z, shadow, A after the event, O).  The host
// zeroes `out` first: the rest stays zero
template <int VT, int AM, bool SKIP>
__global__ __launch_bounds__(kBlock) void isosurface_ao_floats_kernel(const RayMarchParams P, const float* org, const float* dir, float* out, long long n, int max_events, int rotation)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int sub = threadIdx.x & 3;
  const SubMask subm = make_submask(sub);
  VolConsts vc;
  MarchConsts mc;
  setup_consts(P, vc, mc);
  stage_tables<VT, AM>(P, lds_raw, vc);
  __syncthreads();
  const long long i = ((long long)blockIdx.x * kBlock + threadIdx.x) >> 2;
  const bool valid = i < n;
  const long long j = valid ? i : 0;
  const f3 o = mk3(org[3 * j], org[3 * j + 1], org[3 * j + 2]), d = mk3(dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]);
  const f3 oo = to_object(mc, o), od = mk3(d.x * mc.inv_scale.x, d.y * mc.inv_scale.y, d.z * mc.inv_scale.z);
  float t0 = 0.f, t1 = FLT_MAX;
  const bool live = valid && box_test<true>(P, t0, t1, oo, od);
  float* q = out + (8 + 8 * (long long)max_events) * j;
  auto on_event = [&](unsigned int e, int k, float, float, float, float A, const IsoPoint& pt, float O) {
    if (sub != 0 || e >= (unsigned int)max_events) return; // (called by live quads alone: valid holds)
    float* p = q + 8 + 8 * e;
    p[0] = (float)k; p[1] = pt.t; p[2] = pt.n_w.x; p[3] = pt.n_w.y; p[4] = pt.n_w.z; p[5] = pt.shadow; p[6] = A; p[7] = O;
  };
  IsoAo ao;
  const IsoLayers il = isosurface_layers_ao<VT, AM, 2, SKIP, true>(P, vc, mc, o, d, t0, t1, live, rotation & (kAoRotations - 1), subm, ao, on_event);
  const float f = __uint_as_float(ao.fetched);
  const unsigned int ao_fetched = __float_as_uint(quad_bcast<0>(f)) + __float_as_uint(quad_bcast<1>(f)) + __float_as_uint(quad_bcast<2>(f)) + __float_as_uint(quad_bcast<3>(f));
  if (valid && sub == 0) {
    q[0] = (float)il.events; q[1] = il.A; q[2] = live ? (float)il.steps : 0.f; q[3] = (float)il.shadow_steps;
    q[4] = (float)ao.steps; q[5] = (float)ao_fetched; q[6] = 0.f; q[7] = 0.f;
  }
}

// the AO kernels of a voxel type: ONE EXPLICIT INSTANTIATION PER TYPE, in an object of its own (ovr_hip_isosurface.hip with -DOVR_ISO_AO) - the opaque and the
// translucent kernels' objects are compiled from what they were compiled from
typedef void (*IsosurfaceAoFloatsKernel)(const RayMarchParams, const float*, const float*, float*, long long, int, int);
struct IsosurfaceAoKernels { // nullptr: no such variant of this type
  FrameKernel frame = nullptr;
  IsosurfaceAoFloatsKernel floats = nullptr;
};
template <int VT, int AM> struct IsosurfaceAoVariants {
  template <unsigned I> static constexpr IsosurfaceAoKernels at()
  {
    constexpr int shade = (int)(I / kWalkBitsEnd);
    constexpr bool skip = I & kWalkSkip, clipped = I & kWalkClipped, ortho = I & kWalkOrtho;
    if constexpr (!isosurface_variant_exists(shade, AM, skip, clipped, ortho, true, true)) return {};
    else return { isosurface_ao_kernel<VT, AM, shade, skip, ortho>, isosurface_ao_floats_kernel<VT, AM, skip> };
  }
};
// an AO plan's kernels of a voxel type; nullptr for any other plan, for a replica's type and for mode 4 on a layout without row loads
template <int VT>
IsosurfaceAoKernels isosurface_ao_kernels_of(const LaunchPlan& pl)
{
  constexpr unsigned n = 3 * kWalkBitsEnd;
  const unsigned i = (unsigned)pl.shading * kWalkBitsEnd + walk_bits(pl.isosurface.skip, pl.isosurface.clipped, pl.orthographic);
  if (pl.error || !pl.isosurface.on || !pl.isosurface.translucent || !pl.ambient_occlusion || i >= n) return IsosurfaceAoKernels();
  return dispatch_addressing<IsosurfaceAoKernels, VT, true>(pl.am, [&](auto m) {
    return variant_at<IsosurfaceAoVariants<VT, decltype(m)::value>>(i, std::make_integer_sequence<unsigned, n>());
  });
}

} // namespace ovrhip
