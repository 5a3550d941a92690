// ovr_hip_device.h - device code of the ray-march path that depends on the voxel type: helpers, the bricked voxel access,
// raymarch_kernel / shade_pool_kernel and frame_kernels, the lookup from a launch plan (host/launch_plan.hpp) to its two kernels.  Included by
// ovr_hip_kernels.hip (type-independent kernels, the launch sequence) and by ovr_hip_march.hip (one explicit instantiation of frame_kernels, compiled
// once per voxel type).
// See ovr_hip_kernels.hip for the overview.
#pragma once
#include "ovr_hip_kernels.h"

#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include <utility>

namespace ovrhip {

// ------------------------------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------------------------------
struct f3 { float x, y, z; };
__device__ __forceinline__ f3 mk3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ f3 ld3(const float3_& a) { return mk3(a.x, a.y, a.z); }
__device__ __forceinline__ float dot3(f3 a, f3 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }
// clamp(x, lo, hi) for lo <= hi as ONE instruction: v_med3_f32 returns the median of its operands, and min3 of them when one is NaN - with
// IEEE v_min that is the smallest non-NaN operand, lo - so the result equals fminf(fmaxf(x, lo), hi) for every input, NaN -> lo like CUDA's
// fminf / fmaxf (the two-instruction form was ~9 % of the shadow march's instructions, which bound the all-shaded frames)
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return __builtin_amdgcn_fmed3f(x, lo, hi); }
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); } // NaN -> 0 like CUDA fminf/fmaxf (folds into a clamp modifier)
__device__ __forceinline__ float lerpf(float a, float b, float f) { return fmaf(f, b - a, a); }
// gdt normalize (extern/gdt/gdt/math/vec.h:443-448) with the hardware reciprocal square root (1 ulp)
// OVR_PARITY_EXACT = 1 builds the PARITY INSTRUMENT (libovr_hip_parity.so; never the product, nothing loads it by default): the four places where the
// kernels deliberately depart from the oracle's float arithmetic take the oracle's form instead - (1) the opacity correction's __powf is
// the machine-independent det_powf below instead of v_exp_f32(y * v_log_f32(x)), (2) the three per-sample normalisations divide by sqrtf instead of
// multiplying with v_rsq_f32, (3) the gradient divides by the step instead of multiplying with its reciprocal, (4) 8-bit voxels are normalised one by
// one before the filter instead of once behind it.  tests/test_parity_exact_gpu.py: frames and every counter then equal the oracle's (mode "det") - which
// pins those four as the ONLY sources of the product's tolerated differences.
#ifndef OVR_PARITY_EXACT
#define OVR_PARITY_EXACT 0
#endif
__device__ __forceinline__ f3 normalize3(f3 v)
{
#if OVR_PARITY_EXACT
  const float l = sqrtf(dot3(v, v)); // gdt normalize: (v * 1.f) / sqrt(dot(v, v)), extern/gdt/gdt/math/vec.h:443-448
  return mk3(v.x / l, v.y / l, v.z / l);
#endif
  const float r = __builtin_amdgcn_rsqf(dot3(v, v));
  return mk3(v.x * r, v.y * r, v.z * r);
}
// IEEE-exact normalize for the once-per-ray direction
__device__ __forceinline__ f3 normalize3_exact(f3 v)
{
  const float l = sqrtf(dot3(v, v));
  return mk3(v.x / l, v.y / l, v.z / l);
}

// opacity correction, shaders_raymarching.cu:118-122: 1 - __powf(1 - a, base*dt); __powf == exp2(y * log2(x)).
// BF: branch-free form (bit select instead of the exec-mask branch the compiler builds around the two transcendentals);
// same value - adj == 1 keeps a exactly as the reference's branch does.  Only the skipping shadow march gains from it
// (0.85 -> 0.71 ms on C3); the other kernels are measurably slower with it, so they keep the branch.
// A log2 / exp2 pair that is the same float arithmetic on every machine (fmaf Horner chains, integer exponent handling; ~1 ulp each, the accuracy
// class of v_log_f32 / v_exp_f32).  NOT the product's pow: a library built with -DOVR_PARITY_EXACT=1 (libovr_hip_parity.so) evaluates __powf with it, and so
// does the CPU oracle in its mode 2 - with the same pow on both sides every sample count equals the oracle's exactly (tests/test_parity_exact_gpu.py): the
// last bit of the transcendentals is all that the parity tests' remaining tolerances come from.  Constants: tests/golden/make_detpow.py.
__device__ __forceinline__ float det_log2f(float x)
{
  if (!(x > 0.f)) return x == 0.f ? -__builtin_inff() : __builtin_nanf("");
  if (x > 3.402823466e+38f) return x;
  unsigned int ix = __float_as_uint(x);
  int e = (int)(ix >> 23) - 127;
  if (e == -127) { ix = __float_as_uint(x * 8388608.f); e = (int)(ix >> 23) - 127 - 23; }
  float m = __uint_as_float((ix & 0x007fffffu) | 0x3f800000u);
  if (m > 0x1.6a09e6p+0f) { m = m * 0.5f; e += 1; }
  const float f = m - 1.f;
  float p = -0x1.b8f078p-4f;
  p = fmaf(p, f, 0x1.7aec18p-3f);
  p = fmaf(p, f, -0x1.881ca4p-3f);
  p = fmaf(p, f, 0x1.a37bc2p-3f);
  p = fmaf(p, f, -0x1.eab168p-3f);
  p = fmaf(p, f, 0x1.277a9ap-2f);
  p = fmaf(p, f, -0x1.715a9p-2f);
  p = fmaf(p, f, 0x1.ec70a8p-2f);
  p = fmaf(p, f, -0x1.71547p-1f);
  p = fmaf(p, f, 0x1.715476p+0f);
  return fmaf(f, p, (float)e);
}
__device__ __forceinline__ float det_exp2f(float m)
{
  if (m != m) return m;
  if (m >= 128.f) return __builtin_inff();
  if (m < -126.f) return 0.f;
  const float n = floorf(m + 0.5f);
  const float r = m - n;
  float p = 0x1.00c0e4p-16f;
  p = fmaf(p, r, 0x1.446c7ap-13f);
  p = fmaf(p, r, 0x1.5d8776p-10f);
  p = fmaf(p, r, 0x1.3b29d8p-7f);
  p = fmaf(p, r, 0x1.c6b08ep-5f);
  p = fmaf(p, r, 0x1.ebfbep-3f);
  p = fmaf(p, r, 0x1.62e43p-1f);
  p = fmaf(p, r, 1.f);
  const int in = (int)n;
  const int h = in / 2;
  const float s = p * __uint_as_float((unsigned int)(h + 127) << 23) * __uint_as_float((unsigned int)(in - h + 127) << 23);
  return s < 1.175494351e-38f ? 0.f : s;
}
__device__ __forceinline__ float det_powf(float x, float y) { return det_exp2f(y * det_log2f(x)); }
template <bool BF>
__device__ __forceinline__ float opacity_correction(float a, float adj)
{
#if OVR_PARITY_EXACT
  if (!(fabsf(adj - 1.f) < 1e-7f)) a = clamp01(1.f - det_powf(1.f - a, adj));
  return a;
#endif
  if (BF) {
    const float pw = __builtin_amdgcn_exp2f(adj * __builtin_amdgcn_logf(1.f - a));
    const float c = clamp01(1.f - pw);
    const unsigned int m = (fabsf(adj - 1.f) < 1e-7f) ? 0u : ~0u;
    return __uint_as_float((__float_as_uint(c) & m) | (__float_as_uint(a) & ~m));
  }
  if (!(fabsf(adj - 1.f) < 1e-7f)) {
    const float pw = __builtin_amdgcn_exp2f(adj * __builtin_amdgcn_logf(1.f - a));
    a = clamp01(1.f - pw);
  }
  return a;
}

// ------------------------------------------------------------------------------------------------------------------
// voxel access.  Volume layout in HBM: 128-byte bricks with an x-apron, inside macro blocks (see ovr_hip_kernels.h).
// One L1/L2 line is one brick.  A brick stores CX+1 voxels along x (the last one duplicates the first of its +x neighbour),
// so the two x-neighbours of a trilinear tap always sit next to each other in ONE brick and a tap is 4 pair loads
// (f32: 4 x 8 bytes) instead of 8 scalar loads.  The texture addresser spends ~41 clocks on a 64-lane gather instruction
// whatever its width (tools/ubench_gather.hip), so halving the instruction count halves the cost of the path's bottleneck;
// the price is 4/3 (8/7 for 8-bit) of the memory.   f32: (3+1)x4x2   u16/i16: (3+1)x4x4   u8/i8: (7+1)x4x4
// The element offset is separable: off(x,y,z) = X(x) + Y(y) + Z(z).
// ------------------------------------------------------------------------------------------------------------------
typedef float f32x2_u __attribute__((ext_vector_type(2), aligned(4)));
typedef unsigned short u16x2_u __attribute__((ext_vector_type(2), aligned(2)));
typedef short i16x2_u __attribute__((ext_vector_type(2), aligned(2)));
typedef unsigned char u8x2_u __attribute__((ext_vector_type(2), aligned(1)));
typedef signed char i8x2_u __attribute__((ext_vector_type(2), aligned(1)));

template <int VT> struct Vox;
// (the f32 brick shape is what the A/B runs of profiles/r02_notes.md keep)
template <> struct Vox<VOX_F32> {
  typedef float T; typedef f32x2_u P;
  static constexpr int cx = 3, mbx = 10, by = 2, bz = 1; // cells per brick in x, bricks per macro block in x, log2 brick y/z
  static constexpr bool kScale = false, kClamp = false;
  static constexpr bool kTransposed = false;
  static constexpr bool kQuad = false;
};
template <> struct Vox<VOX_U16> {
  typedef unsigned short T; typedef u16x2_u P;
  static constexpr int cx = 3, mbx = 10, by = 2, bz = 2;
  static constexpr bool kScale = false, kClamp = false; // u16 is sampled as RAW float (array.cpp:335-338)
  static constexpr bool kTransposed = false;
  static constexpr bool kQuad = false;
};
// Thin replicas (view-dependent layout choice, see VoxelType in ovr_hip_kernels.h): 1 cell + apron along the pair axis, 4 x 4
// (f32) or 4 x 8 (u16) voxels across.  *_TT is stored with x and y exchanged, so its pair axis is the volume's y.
template <> struct Vox<VOX_F32_T> {
  typedef float T; typedef f32x2_u P;
  static constexpr int cx = 1, mbx = 32, by = 2, bz = 2;
  static constexpr bool kScale = false, kClamp = false;
  static constexpr bool kTransposed = false;
  static constexpr bool kQuad = false;
};
template <> struct Vox<VOX_F32_TT> : Vox<VOX_F32_T> { static constexpr bool kTransposed = true; };
template <> struct Vox<VOX_U16_T> {
  typedef unsigned short T; typedef u16x2_u P;
  static constexpr int cx = 1, mbx = 32, by = 2, bz = 3;
  static constexpr bool kScale = false, kClamp = false;
  static constexpr bool kTransposed = false;
  static constexpr bool kQuad = false;
};
template <> struct Vox<VOX_U16_TT> : Vox<VOX_U16_T> { static constexpr bool kTransposed = true; };
template <> struct Vox<VOX_I16> {
  typedef short T; typedef i16x2_u P;
  static constexpr int cx = 3, mbx = 10, by = 2, bz = 2;
  static constexpr bool kScale = false, kClamp = false;
  static constexpr bool kTransposed = false;
  static constexpr bool kQuad = false;
};
template <> struct Vox<VOX_U8> {
  typedef unsigned char T; typedef u8x2_u P;
  static constexpr int cx = 7, mbx = 4, by = 2, bz = 2;
  static constexpr bool kScale = true, kClamp = false; // normalized read: v / 255 (array.cpp:304-306)
  static constexpr bool kTransposed = false;
  static constexpr bool kQuad = false;
};
template <> struct Vox<VOX_I8> {
  typedef signed char T; typedef i8x2_u P;
  static constexpr int cx = 7, mbx = 4, by = 2, bz = 2;
  static constexpr bool kScale = true, kClamp = true; // max(v / 127, -1)
  static constexpr bool kTransposed = false;
  static constexpr bool kQuad = false;
};

// Quad replicas (VoxelType in ovr_hip_kernels.h): a cell stores its 2 x 2 (x, y) voxels as one 4-vector Q; a 128-byte brick holds
// 2^lx x 2^ly x 2^lz cells.  (cx / mbx / by / bz describe the brick to the code that is shared with the other layouts; P is not used)
typedef float f32x4_q __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4_q __attribute__((ext_vector_type(4)));
typedef unsigned char u8x4_q __attribute__((ext_vector_type(4)));
template <> struct Vox<VOX_F32_Q> {
  typedef float T; typedef f32x2_u P; typedef f32x4_q Q;
  static constexpr int lx = 1, ly = 1, lz = 1;
  static constexpr int cx = 2, mbx = 16, by = 1, bz = 1;
  static constexpr bool kScale = false, kClamp = false;
  static constexpr bool kTransposed = false;
  static constexpr bool kQuad = true;
};
template <> struct Vox<VOX_U16_Q> {
  typedef unsigned short T; typedef u16x2_u P; typedef u16x4_q Q;
  static constexpr int lx = 2, ly = 1, lz = 1;
  static constexpr int cx = 4, mbx = 8, by = 1, bz = 1;
  static constexpr bool kScale = false, kClamp = false;
  static constexpr bool kTransposed = false;
  static constexpr bool kQuad = true;
};
template <> struct Vox<VOX_U8_Q> {
  typedef unsigned char T; typedef u8x2_u P; typedef u8x4_q Q;
  static constexpr int lx = 2, ly = 2, lz = 1;
  static constexpr int cx = 4, mbx = 8, by = 2, bz = 1;
  static constexpr bool kScale = true, kClamp = false; // normalized read like VOX_U8
  static constexpr bool kTransposed = false;
  static constexpr bool kQuad = true;
};

template <int VT> struct BrickMap {
  typedef Vox<VT> V;
  static constexpr unsigned SX = V::cx + 1;                           // stored voxels per brick row (4 or 8)
  static constexpr unsigned BV = SX << (V::by + V::bz);               // stored voxels per brick (128 bytes)
  static constexpr unsigned sby = V::mbx * BV, sbz = (32u >> V::by) * V::mbx * BV;
  static constexpr unsigned MV = (32u >> V::bz) * sbz;                // stored voxels per macro block
  static constexpr unsigned MCX = V::cx * V::mbx;                     // cells per macro block along x (30 or 28)
  static_assert(BV * sizeof(typename V::T) == 128, "a brick is exactly one 128-byte L1/L2 line");
  // exact for x < 65536: q = floor(x / d) = mulhi(x, ceil(2^32 / d))
  static __host__ __device__ __forceinline__ unsigned div_cx(unsigned x) { return (unsigned)(((unsigned long long)x * ((0xffffffffull / V::cx) + 1ull)) >> 32); }
  static __host__ __device__ __forceinline__ unsigned div_mbx(unsigned b) { return (unsigned)(((unsigned long long)b * ((0xffffffffull / V::mbx) + 1ull)) >> 32); }
  // offset of STORED POSITION u as the LOWER member of a pair.  Stored position = voxel index + 1 (round 4): position 0 is a copy of
  // voxel 0, positions past voxel n - 1 repeat it - the pair of voxel index i in [-1, n - 1] is positions (i + 1, i + 2), which is the
  // reference's clamp-to-edge pair (clamp(i), clamp(i + 1)) without a clamp in the tap (shaders_common.h:186-193, cuda_buffer.h:248-287)
  static __host__ __device__ __forceinline__ unsigned X(unsigned x)
  {
    const unsigned b = div_cx(x), xr = x - b * V::cx;
    const unsigned m = div_mbx(b), bm = b - m * V::mbx;
    return xr + bm * BV + m * MV;
  }
  static __host__ __device__ __forceinline__ unsigned Y(unsigned y, unsigned macro_y_stride)
  {
    return (y & ((1u << V::by) - 1u)) * SX + ((y >> V::by) & ((32u >> V::by) - 1u)) * sby + (y >> 5) * macro_y_stride;
  }
  static __host__ __device__ __forceinline__ unsigned Zlo(unsigned z)
  {
    return ((z & ((1u << V::bz) - 1u)) << V::by) * SX + ((z >> V::bz) & ((32u >> V::bz) - 1u)) * sbz;
  }
};

// quad replicas: offsets in voxels (elements of T); cell (u, v, z) -> 4 elements at X(u) + Y(v) + Z(z); cells x-fastest inside a brick, bricks
// x-fastest inside macro blocks of 32^3 cells, macro blocks x-fastest.  Cell (u, v) = (x + 1, y + 1) holds the voxels (clamp(x), clamp(x + 1)) x
// (clamp(y), clamp(y + 1)) for x in [-1, nx - 1], y in [-1, ny - 1] (round 4: the lower faces' clamp-to-edge pairs are cells of their own)
template <int VT> struct QuadMap {
  typedef Vox<VT> V;
  static constexpr unsigned SX = 2, BV = 128u / (unsigned)sizeof(typename V::T);   // elements per brick
  static constexpr unsigned MV = 32u * 32u * 32u * 4u, MCX = 32;                     // elements per macro block; cells per macro block along x
  static constexpr unsigned bx_ = 32u >> V::lx, by_ = 32u >> V::ly;                  // bricks per macro block along x / y
  static_assert((4u << (V::lx + V::ly + V::lz)) == BV, "a brick is exactly one 128-byte L1/L2 line");
  static __host__ __device__ __forceinline__ unsigned div_cx(unsigned x) { return x >> V::lx; }
  static __host__ __device__ __forceinline__ unsigned X(unsigned x) { return (x & ((1u << V::lx) - 1u)) * 4u + ((x >> V::lx) & (bx_ - 1u)) * BV + (x >> 5) * MV; }
  static __host__ __device__ __forceinline__ unsigned Y(unsigned y, unsigned macro_y_stride)
  {
    return (y & ((1u << V::ly) - 1u)) * (4u << V::lx) + ((y >> V::ly) & (by_ - 1u)) * (bx_ * BV) + (y >> 5) * macro_y_stride;
  }
  static __host__ __device__ __forceinline__ unsigned Zlo(unsigned z)
  {
    return (z & ((1u << V::lz) - 1u)) * (4u << (V::lx + V::ly)) + ((z >> V::lz) & ((32u >> V::lz) - 1u)) * (bx_ * by_ * BV);
  }
};
template <> struct BrickMap<VOX_F32_Q> : QuadMap<VOX_F32_Q> {};
template <> struct BrickMap<VOX_U16_Q> : QuadMap<VOX_U16_Q> {};
template <> struct BrickMap<VOX_U8_Q> : QuadMap<VOX_U8_Q> {};

struct VolConsts {
  const void* data;
  // per-axis offset tables in LDS (AM 0 / 1 / 2), bytes (AM 0) or elements (AM 1 / 2).  The pointers are BIASED by one entry: tab_x[i] is
  // valid for the voxel index i = -1 ... n - 1 (lower member of the pair), tab_y[i] / tab_z[i] for i = -1 ... n; index -1 addresses a copy of
  // voxel 0 and index n a copy of voxel n - 1, so (i, i + 1) is the reference's clamp-to-edge pair for every i = floor(x) without a select
  const unsigned int *tab_x, *tab_y, *tab_z;
  const unsigned long long* tab_z64; // AM 2: z offsets need 64 bits (>= 2^32 stored voxels)
  int nx1, ny1, nz1; // n - 1
  const float* majorant; // per-macrocell max TF opacity (null: empty-space skipping off)
  const unsigned char* occupancy; // per 4^3 macrocells: 1 if one of them, or a macrocell next to them, has majorant > 0
  const unsigned char* occupancy_fine; // the same per macrocell
  int mcx1, mcy1, mcz1;  // macrocell grid dims - 1
  unsigned int macro_y;          // stored elements between macro rows: MV * macros_x
  unsigned long long macro_z;    // stored elements between macro layers: MV * macros_x * macros_y
  f3 cs, cb;
  float vscale, vmin;
};

// (int)floor(x) as ONE instruction (the compiler only selects v_cvt_flr_i32_f32 under no-NaNs math; x is never NaN here)
__device__ __forceinline__ int floor_to_int(float x)
{
  int r;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}
// One axis of tex3D's linear filter with clamp addressing (shaders_common.h:186-193; cuda_buffer.h:248-287): x = p * N - 0.5 lies in
// [-0.5, N - 0.5], the texels are (clamp(i0), clamp(i0 + 1)) for i0 = floor(x) in [-1, N - 1], the weight is x - i0.  Every layout stores a
// copy of voxel 0 at index -1 and of voxel N - 1 at index N (in the data along the pair axis, in the offset tables along the others), so
// neither the coordinate nor the indices are clamped (round 4; before, x was clamped to [0, N - 1] and the half voxel outside the first
// centre read (voxel 0, voxel 1) with weight 0 where the reference reads (0, 0): 0 x NaN for a non-finite voxel 1).  In that zone the weight
// is immaterial - lerp(a, a, f) = fma(f, a - a, a) is a for finite a and NaN otherwise, whatever f in [0, 1) - and for x >= 0 v_fract_f32 is the
// exact x - floor(x) of the reference's filter (in full precision: the oracle's convention).
__device__ __forceinline__ void axis_tap(float po, float cs, float cb, int& i0, float& f)
{
  const float p = clamp01(po);                       // sample_volume_object_space clamps p to [0,1] (NaN -> 0)
  const float x = fmaf(p, cs, cb);                   // cell-centred: p*N - 0.5
  f = __builtin_amdgcn_fractf(x);
  i0 = floor_to_int(x);
}

// One trilinear tap, split in two so that several taps can be in flight before the first is consumed
// (software pipelining: the march is latency-bound otherwise).  issue: 4 pair loads; finish: 7 lerps.
struct Tap {
  float c000, c100, c010, c110, c001, c101, c011, c111;
  float fx, fy, fz;
  int x0, y0, z0; // lower corner of the footprint = floor of the texel coordinate, -1 ... n - 1 (live only between tap_coords and tap_loads)
};

// macrocell (16^3 voxels, reference accel/spatial_partition.h:24) whose value range covers the footprint (i0, i0 + 1) on
// every axis: cell c holds voxels [16c - 1, 16c + 15] (sp_singlemc.cu:36-42), i.e. c = (i0 + 1) >> 4

__device__ __forceinline__ void tap_coords(const VolConsts& vc, f3 p, Tap& t)
{
  axis_tap(p.x, vc.cs.x, vc.cb.x, t.x0, t.fx);
  axis_tap(p.y, vc.cs.y, vc.cb.y, t.y0, t.fy);
  axis_tap(p.z, vc.cs.z, vc.cb.z, t.z0, t.fz);
}

__device__ __forceinline__ unsigned int tap_cell(const VolConsts& vc, const Tap& t)
{
  const int cx = min((t.x0 + 1) >> 4, vc.mcx1), cy = min((t.y0 + 1) >> 4, vc.mcy1), cz = min((t.z0 + 1) >> 4, vc.mcz1);
  return (unsigned int)cx + (unsigned int)(vc.mcx1 + 1) * ((unsigned int)cy + (unsigned int)(vc.mcy1 + 1) * (unsigned int)cz);
}

// The pair (x0, x0 + 1) of a brick row.  The texture addresser merges the lanes of a quad that read one 128-byte line only for loads of 8
// bytes or more: a 64-lane gather whose quads each stay inside one line costs 18 clocks as dwordx2 / dwordx4 and 66 - as if every lane had a
// line of its own - as dword or ushort, whatever the alignment (tools/ubench_align.hip, profiles/r05_notes.md section 10; a dwordx2 at a 4-byte
// boundary - the 32-bit bricks' odd pairs - costs the 18; dwords merge only when the quad's four are consecutive).  The 16-bit layouts' pairs are
// 4 bytes: the row loads (RowLoads) read the ALIGNED 8 bytes around the pair (a brick row of the general layout, two rows of a thin replica) and shift the
// pair out of them - the same voxels, so the same frame.  C4: shade 3.21 -> 2.87 ms, frame 7.5 -> 7.2 ms; front view (thin replica) 3.57 -> 3.29;
// a 512^3 u16 volume at 512^2 0.353 -> 0.335; the 8-bit layouts' 2-byte pairs likewise (a 1024^3 u8 volume at C3's settings 1.80 -> 1.70 ms, front view 1.085 ->
// 0.97) - where the layout is large: C1 (256^3 u8) is bound by vector issue and the shifts cost it 3 % (0.183 -> 0.188 ms), see RowLoads.
// Which launches take the row loads: the 16-bit and 8-bit volumes whose layout is too large for the caches to serve (addressing modes 1 and 2, and mode 4 = mode 0's
// 32-bit byte offsets + row loads: plan_launch upgrades a 16-bit or 8-bit layout of more than 128 MB).  Small 16-bit volumes are bound by vector issue and keep the
// 4-byte loads (a 256 x 256 x 226 u16 volume, all samples shaded in place: 0.88 -> 1.08 ms WITH the row loads; the 1024 x 1024 x 1080 one 34 -> 24 ms).
template <int VT, int AM> struct RowLoads { static constexpr bool on = row_load_layout((int)sizeof(typename Vox<VT>::T), Vox<VT>::kQuad) && (AM == 1 || AM == 2 || AM == 4); };
template <int VT, int AM, typename B>
__device__ __forceinline__ typename Vox<VT>::P load_pair(const B* base, unsigned long long off) // off in units of B (bytes for char, else elements)
{
  typedef typename Vox<VT>::T T;
  typedef typename Vox<VT>::P P;
  if constexpr (RowLoads<VT, AM>::on) {
    static_assert(BrickMap<VT>::SX * sizeof(T) <= 8, "row loads: a pair must not cross its aligned 8 bytes, so a brick row is at most 8 bytes");
    constexpr unsigned per = 8u / (unsigned)sizeof(B);                 // units of B per 8 bytes
    const unsigned long long al = off & ~(unsigned long long)(per - 1u);
    const unsigned sh = ((unsigned)off & (per - 1u)) * (8u * (unsigned)sizeof(B));
    const uint2 row = *reinterpret_cast<const uint2*>(base + al);
    const unsigned w = (unsigned)((((unsigned long long)row.y << 32) | (unsigned long long)row.x) >> sh); // (a pair never crosses its 8 bytes: rows are 8 bytes or 4)
    P r;
    if constexpr (sizeof(T) == 2) { r.x = (T)(w & 0xffffu); r.y = (T)(w >> 16); }
    else { r.x = (T)(w & 0xffu); r.y = (T)((w >> 8) & 0xffu); }
    return r;
  }
  else return *reinterpret_cast<const P*>(base + off);
}

// (A non-temporal hint on these loads - `global_load ... nt` - was measured: the march takes 3.50 instead of 1.51 ms, the shade
// kernel 3.17 instead of 1.13 ms on C3: neighbouring quads and consecutive rounds do re-use the lines; profiles/r02_notes.md §7.)
template <int VT, int AM>
__device__ __forceinline__ void tap_loads(const VolConsts& vc, Tap& t)
{
  typedef BrickMap<VT> M;
  typedef typename Vox<VT>::T T;
  typedef typename Vox<VT>::P P;
  if constexpr (Vox<VT>::kQuad) { // quad replica: the (x, y) footprint of a z slice is ONE load (16 / 8 / 4 bytes)
    typedef typename Vox<VT>::Q Q;
    Q q0, q1;
    if (AM == 3) {
      const unsigned z0 = (unsigned)max(t.z0, 0), z1 = (unsigned)min(t.z0 + 1, vc.nz1);
      const unsigned o = M::X((unsigned)(t.x0 + 1)) + M::Y((unsigned)(t.y0 + 1), vc.macro_y);
      const T* base = static_cast<const T*>(vc.data);
      const unsigned long long oz0 = (unsigned long long)M::Zlo(z0) + (unsigned long long)(z0 >> 5) * vc.macro_z;
      const unsigned long long oz1 = (unsigned long long)M::Zlo(z1) + (unsigned long long)(z1 >> 5) * vc.macro_z;
      q0 = *reinterpret_cast<const Q*>(base + (oz0 + o)); q1 = *reinterpret_cast<const Q*>(base + (oz1 + o));
    }
    else if (AM == 2) {
      const unsigned o = vc.tab_x[t.x0] + vc.tab_y[t.y0];
      const unsigned long long oz0 = vc.tab_z64[t.z0], oz1 = vc.tab_z64[t.z0 + 1];
      const T* base = static_cast<const T*>(vc.data);
      q0 = *reinterpret_cast<const Q*>(base + (oz0 + o)); q1 = *reinterpret_cast<const Q*>(base + (oz1 + o));
    }
    else {
      const unsigned o = vc.tab_x[t.x0] + vc.tab_y[t.y0];
      const unsigned oz0 = vc.tab_z[t.z0], oz1 = vc.tab_z[t.z0 + 1];
      if (AM == 1) {
        const T* base = static_cast<const T*>(vc.data);
        q0 = *reinterpret_cast<const Q*>(base + (oz0 + o)); q1 = *reinterpret_cast<const Q*>(base + (oz1 + o));
      }
      else {
        const char* cb = static_cast<const char*>(vc.data);
        q0 = *reinterpret_cast<const Q*>(cb + (oz0 + o)); q1 = *reinterpret_cast<const Q*>(cb + (oz1 + o));
      }
    }
    t.c000 = (float)q0.x; t.c100 = (float)q0.y; t.c010 = (float)q0.z; t.c110 = (float)q0.w;
    t.c001 = (float)q1.x; t.c101 = (float)q1.y; t.c011 = (float)q1.z; t.c111 = (float)q1.w;
    return;
  }
  // layout coordinates (a, b, c): a = the pair axis (the volume's x; its y in a transposed replica), b = the other of the two
  constexpr bool TR = Vox<VT>::kTransposed;
  const int a0 = TR ? t.y0 : t.x0, b0 = TR ? t.x0 : t.y0, z0 = t.z0;
  P p00, p10, p01, p11;
  if (AM == 3) { // > 2^32 elements and axis tables too large for LDS: 64-bit element offsets, computed arithmetically (explicit clamps)
    const int nb1 = TR ? vc.nx1 : vc.ny1;
    const unsigned bc0 = (unsigned)max(b0, 0), bc1 = (unsigned)min(b0 + 1, nb1), zc0 = (unsigned)max(z0, 0), zc1 = (unsigned)min(z0 + 1, vc.nz1);
    const unsigned ox = M::X((unsigned)(a0 + 1));
    const unsigned o0 = ox + M::Y(bc0, vc.macro_y), o1 = ox + M::Y(bc1, vc.macro_y);
    const T* base = static_cast<const T*>(vc.data);
    const unsigned long long oz0 = (unsigned long long)M::Zlo(zc0) + (unsigned long long)(zc0 >> 5) * vc.macro_z;
    const unsigned long long oz1 = (unsigned long long)M::Zlo(zc1) + (unsigned long long)(zc1 >> 5) * vc.macro_z;
    p00 = *reinterpret_cast<const P*>(base + (oz0 + o0)); p10 = *reinterpret_cast<const P*>(base + (oz0 + o1));
    p01 = *reinterpret_cast<const P*>(base + (oz1 + o0)); p11 = *reinterpret_cast<const P*>(base + (oz1 + o1));
  }
  else if (AM == 2) { // > 2^32 elements: a and b offsets (inside one macro layer) stay 32-bit, the z table is 64-bit
    const unsigned ox = vc.tab_x[a0];
    const unsigned o0 = ox + vc.tab_y[b0], o1 = ox + vc.tab_y[b0 + 1];
    const unsigned long long oz0 = vc.tab_z64[z0], oz1 = vc.tab_z64[z0 + 1];
    const T* base = static_cast<const T*>(vc.data);
    p00 = load_pair<VT, AM>(base, oz0 + o0); p10 = load_pair<VT, AM>(base, oz0 + o1);
    p01 = load_pair<VT, AM>(base, oz1 + o0); p11 = load_pair<VT, AM>(base, oz1 + o1);
  }
  else {
    // three LDS lookups (one b32 + two adjacent pairs) replace ~40 bit-field / multiply instructions per tap: the march is
    // VALU-bound once its gathers coalesce, and the LDS pipe is otherwise nearly idle
    const unsigned ox = vc.tab_x[a0];
    const unsigned oy0 = vc.tab_y[b0], oy1 = vc.tab_y[b0 + 1];
    const unsigned oz0 = vc.tab_z[z0], oz1 = vc.tab_z[z0 + 1];
    const unsigned o0 = ox + oy0, o1 = ox + oy1;
    if (AM == 1) { // < 2^32 elements: 32-bit element offsets, one 64-bit shift-add per load
      const T* base = static_cast<const T*>(vc.data);
      p00 = load_pair<VT, AM>(base, (unsigned long long)(oz0 + o0)); p10 = load_pair<VT, AM>(base, (unsigned long long)(oz0 + o1));
      p01 = load_pair<VT, AM>(base, (unsigned long long)(oz1 + o0)); p11 = load_pair<VT, AM>(base, (unsigned long long)(oz1 + o1));
    }
    else { // the whole volume is <= 4 GiB: 32-bit BYTE offsets, the loads use the SGPR-base + 32-bit-VGPR-offset form
      const char* cb = static_cast<const char*>(vc.data);
      p00 = load_pair<VT, AM>(cb, (unsigned long long)(oz0 + o0)); p10 = load_pair<VT, AM>(cb, (unsigned long long)(oz0 + o1));
      p01 = load_pair<VT, AM>(cb, (unsigned long long)(oz1 + o0)); p11 = load_pair<VT, AM>(cb, (unsigned long long)(oz1 + o1));
    }
  }
  // p(b, c) = the pair along a at (b0 + b, z0 + c); the corners keep their volume-axis names, so the lerp order (x, then y,
  // then z) and with it every bit of the result is the same for every layout
  if (!TR) {
    t.c000 = (float)p00.x; t.c100 = (float)p00.y; t.c010 = (float)p10.x; t.c110 = (float)p10.y;
    t.c001 = (float)p01.x; t.c101 = (float)p01.y; t.c011 = (float)p11.x; t.c111 = (float)p11.y;
  }
  else {
    t.c000 = (float)p00.x; t.c010 = (float)p00.y; t.c100 = (float)p10.x; t.c110 = (float)p10.y;
    t.c001 = (float)p01.x; t.c011 = (float)p01.y; t.c101 = (float)p11.x; t.c111 = (float)p11.y;
  }
}

template <int VT, int AM>
__device__ __forceinline__ void tap_issue(const VolConsts& vc, f3 p, Tap& t)
{
  tap_coords(vc, p, t);
  tap_loads<VT, AM>(vc, t);
}

template <int VT>
__device__ __forceinline__ float tap_finish(const VolConsts& vc, Tap t)
{
#if OVR_PARITY_EXACT
  if (Vox<VT>::kScale) { // the texture's normalized read, voxel by voxel: v / 255, max(v / 127, -1) (array.cpp:304-306, array.h:68-106)
    float* c = &t.c000;
    for (int k = 0; k < 8; ++k) c[k] = Vox<VT>::kClamp ? fmaxf(c[k] / 127.f, -1.f) : c[k] / 255.f;
  }
#else
  if (Vox<VT>::kClamp) {
    t.c000 = fmaxf(t.c000, vc.vmin); t.c100 = fmaxf(t.c100, vc.vmin); t.c010 = fmaxf(t.c010, vc.vmin); t.c110 = fmaxf(t.c110, vc.vmin);
    t.c001 = fmaxf(t.c001, vc.vmin); t.c101 = fmaxf(t.c101, vc.vmin); t.c011 = fmaxf(t.c011, vc.vmin); t.c111 = fmaxf(t.c111, vc.vmin);
  }
#endif
  const float c00 = lerpf(t.c000, t.c100, t.fx), c10 = lerpf(t.c010, t.c110, t.fx);
  const float c01 = lerpf(t.c001, t.c101, t.fx), c11 = lerpf(t.c011, t.c111, t.fx);
  const float c0 = lerpf(c00, c10, t.fy), c1 = lerpf(c01, c11, t.fy);
  float s = lerpf(c0, c1, t.fz);
  if (Vox<VT>::kScale && !OVR_PARITY_EXACT) s *= vc.vscale;
  return s;
}

// trilinear tap at object-space p (shaders_common.h:186-193); returns what tex3D<float> returns
template <int VT, int AM>
__device__ __forceinline__ float sample_volume(const VolConsts& vc, f3 p)
{
  Tap t;
  tap_issue<VT, AM>(vc, p, t);
  return tap_finish<VT>(vc, t);
}

// (Quad-cooperative taps - one instruction reading the four pairs of ONE tap, the lerps following the data through DPP - were measured bit-identical and
// slower: C3 shade 0.92 -> 1.08 ms, the transposition is paid in vector instructions; profiles/r05_notes.md section 11.  Packed-FP32 lerps
// (v_pk_fma_f32) likewise cost more issue slots than the scalar v_sub + v_fmac pairs; profiles/r03_notes.md.)

// ------------------------------------------------------------------------------------------------------------------
// transfer function in LDS (or global when it does not fit)
// ------------------------------------------------------------------------------------------------------------------
struct TfConsts {
  const float4* color; // LDS or global
  const float* alpha;
  int nc1, na1;
  float fnc1, fna1;
  float lower, upper, scale;
};

__device__ __forceinline__ float tf_coord(const TfConsts& tf, float sample)
{
  return clamp01((fminf(fmaxf(sample, tf.lower), tf.upper) - tf.lower) * tf.scale); // shaders_common.h:363, :316
}
// (both tables carry one more entry, a copy of their last one - stage_tf - so that (i0, i0 + 1) is the reference's clamp-to-edge pair
// without min(i0 + 1, n - 1): i0 = n - 1 only for v = 1, where the fraction is 0 and lerp(a, a, 0) = a; the two alphas arrive with
// one ds_read2_b32.  Three instructions fewer per lookup, i.e. per shadow sample.)
// PAD = false keeps the two separate reads with min(i0 + 1, n - 1): the POOLED march of the headline (bound by L1 fills, not by instructions)
// is 4 % slower with the paired read - 1.512 -> 1.577 ms on C3, same box, four alternating runs (profiles/r03_ab/r03_ab_regress2.txt) - while every
// instruction-bound kernel gains 1-4 % from it (shadow march at rate 4, the in-place kernels of the shipped scenes, C2, C5)
template <bool PAD = true>
__device__ __forceinline__ float tf_alpha(const TfConsts& tf, float v)
{
  const float x = v * tf.fna1;                      // v in [0, 1]: x >= 0, see axis_tap
  const int i0 = (int)x;
  if (!PAD) return lerpf(tf.alpha[i0], tf.alpha[min(i0 + 1, tf.na1)], __builtin_amdgcn_fractf(x));
  return lerpf(tf.alpha[i0], tf.alpha[i0 + 1], __builtin_amdgcn_fractf(x));
}
__device__ __forceinline__ f3 tf_color(const TfConsts& tf, float v)
{
  const float x = v * tf.fnc1;
  const int i0 = (int)x;
  const float f = __builtin_amdgcn_fractf(x);
  const float4 a = tf.color[i0], b = tf.color[i0 + 1];
  return mk3(lerpf(a.x, b.x, f), lerpf(a.y, b.y, f), lerpf(a.z, b.z, f));
}

// ------------------------------------------------------------------------------------------------------------------
// box test vs [0,1]^3, shaders_common.h:156-184 (__frcp_rn restated as an IEEE divide)
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool intersect_unit_box(float& t0, float& t1, f3 o, f3 d)
{
  const bool sx = fabsf(d.x) < FLT_MIN, sy = fabsf(d.y) < FLT_MIN, sz = fabsf(d.z) < FLT_MIN;
  const float rx = 1.f / d.x, ry = 1.f / d.y, rz = 1.f / d.z;
  const float lx = sx ? FLT_MAX : (0.f - o.x) * rx, ly = sy ? FLT_MAX : (0.f - o.y) * ry, lz = sz ? FLT_MAX : (0.f - o.z) * rz;
  const float hx = sx ? -FLT_MAX : (1.f - o.x) * rx, hy = sy ? -FLT_MAX : (1.f - o.y) * ry, hz = sz ? -FLT_MAX : (1.f - o.z) * rz;
  t0 = fmaxf(t0, fmaxf(fmaxf(fminf(lx, hx), fminf(ly, hy)), fminf(lz, hz)));
  t1 = fminf(t1, fminf(fminf(fmaxf(lx, hx), fmaxf(ly, hy)), fmaxf(lz, hz)));
  return t1 > t0;
}
// The reference's quirk, restated above: a direction component below FLT_MIN switches its slab OFF - such a ray "hits" the box wherever
// its origin lies along that axis.  True for a ray that takes this path with its origin outside the ignored slab: the only rays that can
// hit the box from outside its silhouette (the host needs to know: mapframe(HOST) copies the silhouette's rectangle, ovr_hip_api.cpp)
__device__ __forceinline__ bool ignored_slab_outside(f3 o, f3 d)
{
  return (fabsf(d.x) < FLT_MIN && !(o.x >= 0.f && o.x <= 1.f)) || (fabsf(d.y) < FLT_MIN && !(o.y >= 0.f && o.y <= 1.f)) ||
         (fabsf(d.z) < FLT_MIN && !(o.z >= 0.f && o.z <= 1.f));
}

// The clip box (include/ovr_hip.h ovr_hip_set_clip_box; open-volume-renderer_amd/clipping.py is the normative arithmetic): the same test against
// [lo, hi] instead of [0, 1] per axis - the expressions above, operation for operation, with the literal 0.f replaced by lo_k and 1.f by hi_k, so
// that lo = 0, hi = 1 returns the bits intersect_unit_box returns.  An empty box (lo_k >= hi_k on an axis) is missed by every ray, also by one whose
// slab on that axis is ignored.
__device__ __forceinline__ bool intersect_bounds_box(float& t0, float& t1, f3 o, f3 d, f3 lo, f3 hi)
{
  const bool sx = fabsf(d.x) < FLT_MIN, sy = fabsf(d.y) < FLT_MIN, sz = fabsf(d.z) < FLT_MIN;
  const float rx = 1.f / d.x, ry = 1.f / d.y, rz = 1.f / d.z;
  const float lx = sx ? FLT_MAX : (lo.x - o.x) * rx, ly = sy ? FLT_MAX : (lo.y - o.y) * ry, lz = sz ? FLT_MAX : (lo.z - o.z) * rz;
  const float hx = sx ? -FLT_MAX : (hi.x - o.x) * rx, hy = sy ? -FLT_MAX : (hi.y - o.y) * ry, hz = sz ? -FLT_MAX : (hi.z - o.z) * rz;
  t0 = fmaxf(t0, fmaxf(fmaxf(fminf(lx, hx), fminf(ly, hy)), fminf(lz, hz)));
  t1 = fminf(t1, fminf(fminf(fmaxf(lx, hx), fmaxf(ly, hy)), fmaxf(lz, hz)));
  const bool empty = lo.x >= hi.x || lo.y >= hi.y || lo.z >= hi.z;
  return t1 > t0 && !empty;
}
__device__ __forceinline__ bool ignored_slab_outside_bounds(f3 o, f3 d, f3 lo, f3 hi)
{
  return (fabsf(d.x) < FLT_MIN && !(o.x >= lo.x && o.x <= hi.x)) || (fabsf(d.y) < FLT_MIN && !(o.y >= lo.y && o.y <= hi.y)) ||
         (fabsf(d.z) < FLT_MIN && !(o.z >= lo.z && o.z <= hi.z));
}
// CLIP = false is the state without a clip box with its bounds as literals: the kernels every frame runs until ovr_hip_set_clip_box is called are
// the ones that existed before it did (the route of MAT, shade_light below).  The bounds are kernel arguments behind every
// other one (RayMarchParams::clip_lo / clip_hi): scalar registers.
template <bool CLIP>
__device__ __forceinline__ bool box_test(const RayMarchParams& P, float& t0, float& t1, f3 o, f3 d)
{
  if (CLIP) return intersect_bounds_box(t0, t1, o, d, mk3(P.clip_lo.x, P.clip_lo.y, P.clip_lo.z), mk3(P.clip_hi.x, P.clip_hi.y, P.clip_hi.z));
  return intersect_unit_box(t0, t1, o, d);
}
template <bool CLIP>
__device__ __forceinline__ bool box_ignored_slab_outside(const RayMarchParams& P, f3 o, f3 d)
{
  if (CLIP) return ignored_slab_outside_bounds(o, d, mk3(P.clip_lo.x, P.clip_lo.y, P.clip_lo.z), mk3(P.clip_hi.x, P.clip_hi.y, P.clip_hi.z));
  return ignored_slab_outside(o, d);
}

// ------------------------------------------------------------------------------------------------------------------
// TEA, random.h:146-188
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tea16(unsigned int& v0, unsigned int& v1)
{
  unsigned int sum = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    sum += 0x9e3779b9u;
    v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + sum) ^ ((v1 >> 5) + 0xc8013ea4u);
    v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + sum) ^ ((v0 >> 5) + 0x7e95761eu);
  }
}
#define OVR_TEA_TOFLOAT 2.3283064365386962890625e-10f

// ------------------------------------------------------------------------------------------------------------------
// per-frame constants shared by the primary and the shadow march
// ------------------------------------------------------------------------------------------------------------------
struct MarchConsts {
  f3 inv_scale, wto_p, otw_it, light;
  f3 gstep;     // one voxel in normalized object coordinates
  f3 ginv;      // 1 / gstep
  float step, base, shadow_stride;
};

__device__ __forceinline__ f3 to_object(const MarchConsts& mc, f3 p)
{
  return mk3(fmaf(p.x, mc.inv_scale.x, mc.wto_p.x), fmaf(p.y, mc.inv_scale.y, mc.wto_p.y), fmaf(p.z, mc.inv_scale.z, mc.wto_p.z));
}

// The ray of a pixel sample at the screen offsets (ux, uy) = (sx - 0.5, sy - 0.5), in world space (open-volume-renderer_amd/camera.py is the normative
// arithmetic): the ONE statement of it - the frame kernels, the schedule's kernels and ovr_hip_camera_rays call this.
// Perspective: every ray starts at cam_pos - wave-uniform, scalar registers - and the direction is normalised per sample.  ORTHO (the orthographic camera,
// ovr_hip_set_camera_orthographic): every ray has cam_dir's bits as stored, and the origin is the direction expression with the roles of position and
// direction swapped - per lane, which is why it is a compile-time variant: the kernels of a perspective frame never hold it.
template <bool ORTHO>
__device__ __forceinline__ void pixel_ray(const RayMarchParams& P, float ux, float uy, f3& org, f3& dir)
{
  const f3 cpos = ld3(P.cam_pos), cdir = ld3(P.cam_dir), chor = ld3(P.cam_hor), cver = ld3(P.cam_ver);
  if (ORTHO) {
    org = mk3(cpos.x + ux * chor.x + uy * cver.x, cpos.y + ux * chor.y + uy * cver.y, cpos.z + ux * chor.z + uy * cver.z);
    dir = cdir;
  }
  else {
    org = cpos;
    dir = normalize3_exact(mk3(cdir.x + ux * chor.x + uy * cver.x, cdir.y + ux * chor.y + uy * cver.y, cdir.z + ux * chor.z + uy * cver.z));
  }
}
// Does a primary ray meet the box?  Perspective: the reference's test, its quirk included.  ORTHO: a ray through an ignored slab with its origin outside that
// slab is a MISS - under a camera along a volume axis EVERY ray has two such components, and the reference's rule would smear the edge voxels over the
// whole image.  The orthographic kernels exist on the clipped test alone (CLIP = true; the unit box without a clip box)
template <bool CLIP, bool ORTHO>
__device__ __forceinline__ bool primary_box_test(const RayMarchParams& P, float& t0, float& t1, f3 oo, f3 od)
{
  static_assert(!ORTHO || CLIP, "the orthographic variants exist exactly where the clipped ones exist (host/launch_plan.hpp)");
  const bool hit = box_test<CLIP>(P, t0, t1, oo, od);
  if (ORTHO) return hit && !box_ignored_slab_outside<CLIP>(P, oo, od);
  return hit;
}

// Does the ray of pixel (ix, iy) - one sample per pixel, no jitter - meet the volume's box?  The expressions are the march's own
// (raymarch_kernel: screen position, pixel_ray, object-space ray, box test), so the answer is the march's answer bit for bit, the
// ignored-slab quirk of the reference's box test included.  launch_schedule uses it to find the 8x8 blocks NONE of whose rays hits.
template <bool CLIP = false, bool ORTHO = false>
__device__ __forceinline__ bool pixel_ray_hits_box(const RayMarchParams& P, const MarchConsts& mc, int ix, int iy)
{
  const float rsx = 1.f / (float)P.width, rsy = 1.f / (float)P.height;
  const float sx = ((float)ix + .5f) * rsx, sy = ((float)iy + .5f) * rsy;
  const float ux = sx - 0.5f, uy = sy - 0.5f;
  f3 org, dir;
  pixel_ray<ORTHO>(P, ux, uy, org, dir);
  const f3 od = mk3(dir.x * mc.inv_scale.x, dir.y * mc.inv_scale.y, dir.z * mc.inv_scale.z);
  const f3 oo = to_object(mc, org);
  float t0 = 0.f, t1 = FLT_MAX;
  return primary_box_test<CLIP, ORTHO>(P, t0, t1, oo, od);
}

// Empty-space skipping, per ray: the t interval outside of which every sample lies in a macrocell with majorant 0.
// skip_walk: one lane walks the ray's [ta, tb] through an occupancy grid (3-D DDA; accel/dda.h is the reference's walker for
// its path tracer) and widens [first, last] by the entry / exit of every set entry it crosses.  FINE = false: the coarse grid
// (4^3 macrocells = 64 voxels per entry), FINE = true: one entry per macrocell (16 voxels); both are dilated by one macrocell.
// Sample coordinates: x = p * cs + cb (tap_coords), macrocell = (floor(x) + 1) >> 4 (tap_cell), i.e. the regular 16-voxel
// grid in w = x + 1.
// Besides the hull [first, last] a span carries a 64-bit mask over 64 equal segments of [seg0, seg0 + 64 / seg_scale].  Nothing refines the mask any
// more (the segment walker that did was measured 2-4 % slower on every bench configuration, profiles/r03_notes.md): it is all set or all clear.  Its
// fields and tests stay because removing them changes the skipping kernels' code - that waits for a change that is measured.
struct SkipSpan {
  float first, last;            // hull: every sample outside it lies in a macrocell with majorant 0
  float seg0, seg_scale;        // segment i covers t in [seg0 + i / seg_scale, seg0 + (i + 1) / seg_scale)
  unsigned int mask_lo, mask_hi; // segments that can hold a sample with majorant > 0 (all set: no refinement)
};
__device__ __forceinline__ SkipSpan skipspan_all() { SkipSpan s; s.first = -FLT_MAX; s.last = FLT_MAX; s.seg0 = 0.f; s.seg_scale = 0.f; s.mask_lo = s.mask_hi = ~0u; return s; }
__device__ __forceinline__ SkipSpan skipspan_none() { SkipSpan s; s.first = FLT_MAX; s.last = -FLT_MAX; s.seg0 = 0.f; s.seg_scale = 0.f; s.mask_lo = s.mask_hi = 0u; return s; }
__device__ __forceinline__ int skipspan_seg(const SkipSpan& s, float t) { return min(max((int)((t - s.seg0) * s.seg_scale), 0), 63); }
// can a sample at t lie in a macrocell with majorant > 0?
__device__ __forceinline__ bool skipspan_inside(const SkipSpan& s, float t)
{
  const int g = skipspan_seg(s, t);
  const unsigned int w = g < 32 ? s.mask_lo : s.mask_hi;
  return t >= s.first && t <= s.last && ((w >> (g & 31)) & 1u) != 0u;
}
// may the t range [ta, tb] (ta <= tb) hold such a sample?
__device__ __forceinline__ bool skipspan_touches(const SkipSpan& s, float ta, float tb)
{
  if (tb < s.first || ta > s.last) return false;
  const int lo = skipspan_seg(s, ta), hi = skipspan_seg(s, tb);
  const unsigned long long m = ((unsigned long long)s.mask_hi << 32) | s.mask_lo;
  const unsigned long long range = (hi >= 63 ? ~0ull : ((2ull << hi) - 1ull)) & ~((1ull << lo) - 1ull);
  return (m & range) != 0ull;
}

template <bool FINE>
__device__ __forceinline__ void skip_walk(const VolConsts& vc, f3 oo, f3 od, float ta, float tb, float& first, float& last)
{
  const float w0[3] = { fmaf(oo.x, vc.cs.x, vc.cb.x + 1.f), fmaf(oo.y, vc.cs.y, vc.cb.y + 1.f), fmaf(oo.z, vc.cs.z, vc.cb.z + 1.f) };
  const float dw[3] = { od.x * vc.cs.x, od.y * vc.cs.y, od.z * vc.cs.z };
  const int m1[3] = { FINE ? vc.mcx1 : vc.mcx1 >> 2, FINE ? vc.mcy1 : vc.mcy1 >> 2, FINE ? vc.mcz1 : vc.mcz1 >> 2 }; // grid dims - 1
  const unsigned char* grid = FINE ? vc.occupancy_fine : vc.occupancy;
  constexpr float G = FINE ? 16.f : 64.f;
  int ci[3], st[3];
  float tmax[3], tdel[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float w = fmaf(ta, dw[k], w0[k]);
    ci[k] = min(max((int)floorf(w * (1.f / G)), 0), m1[k]);
    st[k] = dw[k] > 0.f ? 1 : -1;
    const bool moves = fabsf(dw[k]) > 1e-20f;
    tdel[k] = moves ? G / fabsf(dw[k]) : FLT_MAX;
    tmax[k] = moves ? ((float)(ci[k] + (dw[k] > 0.f ? 1 : 0)) * G - w0[k]) / dw[k] : FLT_MAX;
  }
  float t = ta;
  const int limit = m1[0] + m1[1] + m1[2] + 8; // a ray crosses at most this many entries: every lane leaves the loop
  for (int it = 0; it < limit && t < tb; ++it) {
    const bool occ = grid[(size_t)ci[0] + (size_t)(m1[0] + 1) * ((size_t)ci[1] + (size_t)(m1[1] + 1) * (size_t)ci[2])] != 0;
    const int ax = (tmax[0] <= tmax[1]) ? (tmax[0] <= tmax[2] ? 0 : 2) : (tmax[1] <= tmax[2] ? 1 : 2);
    const float tn = ax == 0 ? tmax[0] : ax == 1 ? tmax[1] : tmax[2];
    if (occ) { first = fminf(first, t); last = fmaxf(last, fminf(tn, tb)); }
    t = fmaxf(t, tn);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k == ax) {
        const int nxt = ci[k] + st[k];
        if (nxt < 0 || nxt > m1[k]) tmax[k] = FLT_MAX; // the clamped coordinate stays in the border entry
        else { ci[k] = nxt; tmax[k] += tdel[k]; }
      }
  }
  if (t < tb) { first = fminf(first, t); last = tb; } // safety limit hit (never expected): treat the rest as occupied
}

// raymarching_shadow, shaders_raymarching.cu:44-85 (+ :205-229): alpha-only march toward the light.
// KS taps are issued before the first one is consumed; taps past the end of the march or past the early-termination
// point are speculative (their coordinates are clamped, so the loads are always in bounds) and simply dropped.
// CLIP: the shadow ray is cut by the clip box like the primary ray - what is cut away casts no shadow
template <int VT, int AM, int KS, bool SKIP, bool CLIP = false>
__device__ __forceinline__ float march_shadow(const RayMarchParams& P, const VolConsts& vc, const TfConsts& tf, const MarchConsts& mc, f3 org, unsigned int& n_shadow,
                                              unsigned int& n_shadow_skipped)
{
  const f3 oo = to_object(mc, org);
  const f3 od = mk3(mc.light.x * mc.inv_scale.x, mc.light.y * mc.inv_scale.y, mc.light.z * mc.inv_scale.z);
  float t0 = 0.f, t1 = FLT_MAX;
  float alpha = 0.f;
  if (!box_test<CLIP>(P, t0, t1, oo, od)) return alpha;
  float tx = t0, ty = fminf(t1, t0 + mc.shadow_stride);
  bool live = true;
  // empty-space skipping: the shadow ray's own skip interval (a handful of coarse entries: the ray is a few hundred voxels)
  float skip_first = FLT_MAX, skip_last = -FLT_MAX;
  if (SKIP) skip_walk<false>(vc, oo, od, t0, t1, skip_first, skip_last);
  while (live) {
    Tap taps[KS];
    float dts[KS], mj[KS];
    bool valid[KS];
    bool any_inside = false;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      valid[k] = ty > tx;
      dts[k] = ty - tx;
      const float tm = 0.5f * (tx + ty);
      const bool inside = !SKIP || (tm >= skip_first && tm <= skip_last);
      if (SKIP) taps[k] = Tap{};
      mj[k] = SKIP ? 0.f : 1.f;
      if (inside) {
        const f3 pos = mk3(fmaf(tm, mc.light.x, org.x), fmaf(tm, mc.light.y, org.y), fmaf(tm, mc.light.z, org.z));
        tap_coords(vc, to_object(mc, pos), taps[k]);
        if (SKIP) mj[k] = vc.majorant[tap_cell(vc, taps[k])]; // empty-space skipping: max TF opacity of the macrocell
      }
      any_inside = any_inside || (mj[k] > 0.f);
      tx = ty;
      ty = fminf(tx + mc.shadow_stride, t1);
    }
    if (SKIP && __ballot(any_inside) == 0ull) { // nothing to fetch for any lane of the wave: bookkeeping only
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        live = live && valid[k] && (alpha < 0.9999f);
        n_shadow_skipped += live ? 1u : 0u;
      }
      continue;
    }
#pragma unroll
    for (int k = 0; k < KS; ++k)
      if (!SKIP || mj[k] > 0.f) tap_loads<VT, AM>(vc, taps[k]);
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      // branch-free on purpose: a conditional use would let the compiler sink this tap's loads into the branch and
      // serialise the taps again (seen in the ISA); dead lanes just compute a value that is not used
      const float s = tap_finish<VT>(vc, taps[k]);
      float a = tf_alpha(tf, tf_coord(tf, s));
      a = opacity_correction<SKIP>(a, mc.base * dts[k]);
      if (SKIP) a = mj[k] > 0.f ? a : 0.f; // a macrocell whose majorant is 0 holds no sample with opacity > 0
      live = live && valid[k] && (alpha < 0.9999f);
      alpha = live ? fmaf(1.f - alpha, a, alpha) : alpha;
      n_shadow += (live && (!SKIP || mj[k] > 0.f)) ? 1u : 0u;
      if (SKIP) n_shadow_skipped += (live && !(mj[k] > 0.f)) ? 1u : 0u;
    }
  }
  return alpha;
}

// ------------------------------------------------------------------------------------------------------------------
// the ray-march kernels
//
// Work decomposition: four lanes per ray (a quad = 4 consecutive steps), 16 rays = a 4x4 pixel tile per wave64, four waves
// = 8x8 pixels per workgroup; workgroups are launched longest rays first (launch_schedule).  Details at raymarch_kernel.
//  * primary march: K instructions x 4 steps per round, all their voxel loads in flight before the first is consumed.
//  * deferred, compacted shading (SHADE != 0): a sample whose opacity is > 0 is not shaded by its own lane; the lane
//    pushes a 32-byte request into its wave's queue in LDS (slot = tail + prefix-of-ballot, v_mbcnt) and keeps
//    marching - alpha does not depend on shading, so early termination is unaffected.  Requests are shaded 64 at a
//    time, one request per lane (gradient taps, normals, shadow march toward the light - the expensive, otherwise
//    badly divergent part); each owner applies its colour contributions in sample order (the requests of one lane
//    form a linked list), so the result is bit-identical to shading in place.
//  * two ways to shade a batch:
//      in place   (raymarch_kernel)  the wave that owns the tile shades its own batches and gets the contributions
//                                    back with ds_bpermute.  Used when shading is off and as the reference pipeline.
//      pooled     (raymarch_kernel<POOLED> -> shade_pool_kernel -> composite_kernel)  the tile's wave spills each full
//                                    batch as a 2 KiB chunk into a global pool; a second, persistent kernel shades
//                                    chunks from ALL tiles with perfect load balance (the shadow work of a frame sits in
//                                    a few hundred tiles: in place, their waves ran alone for 10 ms of a 13 ms kernel);
//                                    a third kernel walks each tile's chunks in order and composites.
//  * counters: per-workgroup partial sums, reduced by a tiny kernel (no same-address atomics).
// ------------------------------------------------------------------------------------------------------------------
// (kBlock = 256 threads, kWaves = 4: host/launch_plan.hpp, with the other sizes the launch decision reads)
constexpr int kShadowTaps = 4; // shadow-march taps in flight per lane
// chunks a tile reserves at a time: consecutive chunks of one tile are shaded by ONE workgroup, one chunk per wave
// (L1/L2 reuse: measured 2.4 -> 1.5 ms for the shading kernel at C3; 8 / 16 / 32 are slower - imbalance)
constexpr int kRun = 4;
constexpr int kTicketRuns = 8; // shade kernel: most runs a workgroup takes per ticket
constexpr unsigned int kTicketBlock = 8; // shade kernel: consecutive tickets that stay in one sub-pool
constexpr int kRunMax = 16; // largest reservation (a multiple of kRun: the shade kernel takes kRun chunks per workgroup)

struct ShadeReq { // 32 bytes; after shading the same slot holds the result (cx,cy,cz,gx,gy,gz,a,next)
  float px, py, pz; // world-space sample position          | colour contribution  tr*clamp01(rgb*shade)
  float s;          // sample value                           | gradient contribution tr*clamp01(n_c) .x
  float v;          // transfer-function coordinate           | .y
  float tr;         // transmittance before the sample        | .z
  float a;          // corrected opacity
  int next;         // stream position of the owner's next request (valid once that request exists)
};
static_assert(sizeof(ShadeReq) == kShadeReqBytes, "launch_plan.hpp restates the request's size");

__device__ __forceinline__ float bperm(int src_lane, float x)
{
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(x)));
}
__device__ __forceinline__ int bperm_i(int src_lane, int x) { return __builtin_amdgcn_ds_bpermute(src_lane << 2, x); }

// shade order by light beams (PoolDesc): the beam a world-space position projects into, permuted so that the beams of one XCD list are
// contiguous: list = (cu + 3 cv) % 8 - neighbours in both directions go to different lists -, index = list * G*G/8 + cv * G/8 + cu / 8
__device__ __forceinline__ unsigned int beam_index(const PoolDesc& Q, float px, float py, float pz)
{
  const int G = Q.order_grid;
  const int cu = min(max((int)fmaf(px, Q.order_u[0], fmaf(py, Q.order_u[1], fmaf(pz, Q.order_u[2], Q.order_u[3]))), 0), G - 1); // (NaN -> 0)
  const int cv = min(max((int)fmaf(px, Q.order_v[0], fmaf(py, Q.order_v[1], fmaf(pz, Q.order_v[2], Q.order_v[3]))), 0), G - 1);
  return ((unsigned int)(cu + 3 * cv) & 7u) * (unsigned int)(G * G / 8) + (unsigned int)(cv * (G / 8) + (cu >> 3));
}

__device__ __forceinline__ void setup_consts(const RayMarchParams& P, VolConsts& vc, MarchConsts& mc)
{
  vc.data = P.vol.data;
  vc.nx1 = P.vol.nx - 1; vc.ny1 = P.vol.ny - 1; vc.nz1 = P.vol.nz - 1;
  vc.macro_y = P.vol.macro_elems * (unsigned int)P.vol.macros_x;
  vc.macro_z = (unsigned long long)P.vol.macro_elems * (unsigned long long)P.vol.macros_x * (unsigned long long)P.vol.macros_y;
  vc.cs = ld3(P.coord_scale); vc.cb = ld3(P.coord_bias);
  vc.vscale = P.vol.value_scale; vc.vmin = P.vol.value_min_clamp;
  vc.majorant = P.majorant;
  vc.occupancy = P.occupancy;
  vc.occupancy_fine = P.occupancy_fine;
  vc.mcx1 = (P.vol.nx + 15) / 16 - 1; vc.mcy1 = (P.vol.ny + 15) / 16 - 1; vc.mcz1 = (P.vol.nz + 15) / 16 - 1;
  mc.inv_scale = ld3(P.inv_scale); mc.wto_p = ld3(P.wto_p); mc.otw_it = ld3(P.otw_it); mc.light = ld3(P.light);
  mc.gstep = ld3(P.grad_step);
  mc.ginv = mk3(1.f / mc.gstep.x, 1.f / mc.gstep.y, 1.f / mc.gstep.z);
  mc.step = P.step; mc.base = P.base; mc.shadow_stride = P.shadow_stride;
}

// copy the layout's per-axis offset tables (VolumeDesc::axis_ab / axis_z, built once per volume by axis_tables_kernel) into LDS,
// scaled to what the addressing mode adds to its base (all threads of the workgroup); returns the bytes used
template <int VT, int AM>
__device__ __forceinline__ size_t stage_tables(const RayMarchParams& P, unsigned char* base, VolConsts& vc)
{
  vc.tab_x = vc.tab_y = vc.tab_z = nullptr;
  vc.tab_z64 = nullptr;
  if (AM == 3) return 0;
  // layout axes: a = pair axis, b = the other one (x and y, exchanged in a transposed replica)
  const int na = Vox<VT>::kTransposed ? P.vol.ny : P.vol.nx, nb = Vox<VT>::kTransposed ? P.vol.nx : P.vol.ny;
  const unsigned int* __restrict__ gab = P.vol.axis_ab;
  const unsigned long long* __restrict__ gz = P.vol.axis_z;
  const int ea = axis_a_entries(na), nab = ea + axis_b_entries(nb), ez = axis_z_entries(P.vol.nz);
  // the table pointers handed to the taps are biased by one entry: index -1 is entry 0 (see VolConsts)
  if (AM == 2) { // [z: ez x u64][a: ea x u32][b: eb x u32], element offsets: the global tables as they are
    unsigned long long* tz = reinterpret_cast<unsigned long long*>(base);
    unsigned int* tx = reinterpret_cast<unsigned int*>(tz + ez);
    for (int i = threadIdx.x; i < nab; i += kBlock) tx[i] = gab[i];
    for (int i = threadIdx.x; i < ez; i += kBlock) tz[i] = gz[i];
    vc.tab_x = tx + 1; vc.tab_y = tx + ea + 1; vc.tab_z64 = tz + 1;
    return (size_t)ez * sizeof(unsigned long long) + (size_t)nab * sizeof(unsigned int);
  }
  // AM 0: byte offsets (the volume is <= 4 GiB), AM 1: element offsets (< 2^32 stored voxels) - 32 bits hold every entry
  unsigned int* tx = reinterpret_cast<unsigned int*>(base);
  unsigned int* tz = tx + nab;
  const unsigned int mul = (AM == 0 || AM == 4) ? (unsigned int)sizeof(typename Vox<VT>::T) : 1u;
  for (int i = threadIdx.x; i < nab; i += kBlock) tx[i] = gab[i] * mul;
  for (int i = threadIdx.x; i < ez; i += kBlock) tz[i] = (unsigned int)gz[i] * mul;
  vc.tab_x = tx + 1; vc.tab_y = tx + ea + 1; vc.tab_z = tz + 1;
  return (size_t)(nab + ez) * sizeof(unsigned int);
}
// stage the transfer function in LDS (all threads of the workgroup); color may be skipped by alpha-only kernels
__device__ __forceinline__ void stage_tf(const RayMarchParams& P, unsigned char* tf_base, bool with_color, TfConsts& tf)
{
  float4* lc = reinterpret_cast<float4*>(tf_base);
  float* la = reinterpret_cast<float*>(tf_base + (with_color ? (size_t)(P.n_color + 1) * sizeof(float4) : 0));
  if (with_color) {
    const float4* gc = reinterpret_cast<const float4*>(P.tf_color);
    for (int i = threadIdx.x; i <= P.n_color; i += kBlock) lc[i] = gc[min(i, P.n_color - 1)]; // one more entry, a copy of the last (tf_color)
  }
  for (int i = threadIdx.x; i < P.n_alpha; i += kBlock) la[i] = P.tf_alpha[i];
  if (threadIdx.x == 0) la[P.n_alpha] = P.tf_alpha[P.n_alpha - 1]; // one more entry, a copy of the last: (i, i + 1) is clamp-to-edge (tf_alpha)
  __syncthreads();
  tf.color = lc;
  tf.alpha = la;
  tf.nc1 = P.n_color - 1; tf.na1 = P.n_alpha - 1;
  tf.fnc1 = (float)tf.nc1; tf.fna1 = (float)tf.na1;
  tf.lower = P.tf_lower; tf.upper = P.tf_upper; tf.scale = P.tf_scale;
}

// accumulation + framebuffer write, shaders_raymarching.cu:389-409
__device__ __forceinline__ void write_pixel(const RayMarchParams& P, unsigned int pixel_index, f3 o_c, float o_a, f3 o_g)
{
  float4 out = make_float4(o_c.x, o_c.y, o_c.z, o_a);
  float4* fb = reinterpret_cast<float4*>(P.rgba) + pixel_index;
  if (P.accumulate) {
    float4* ac = reinterpret_cast<float4*>(P.accum) + pixel_index;
    if (P.accum_half && (P.frame_index & 1) == 0) { // convergence estimate: H = the sum of the even-numbered frames, kept exactly as A is
      float4* hp = reinterpret_cast<float4*>(P.accum_half) + pixel_index;
      if (P.frame_index == 2) {
        *hp = out;
      }
      else {
        float4 h = *hp;
        h.x += out.x; h.y += out.y; h.z += out.z; h.w += out.w;
        *hp = h;
      }
    }
    if (P.frame_index == 1) {
      *ac = out;
    }
    else {
      float4 acc = *ac;
      acc.x += out.x; acc.y += out.y; acc.z += out.z; acc.w += out.w;
      *ac = acc;
      const float fi = (float)P.frame_index;
      out = make_float4(acc.x / fi, acc.y / fi, acc.z / fi, acc.w / fi);
    }
  }
  *fb = out;
  if (P.grad) {
    float* pg = P.grad + 3ull * pixel_index;
    pg[0] = o_g.x; pg[1] = o_g.y; pg[2] = o_g.z;
  }
}

// The shade factor (include/ovr_hip.h ovr_hip_set_light / ovr_hip_set_material; open-volume-renderer_amd/lighting.py is the normative arithmetic), in
// two steps so that shade_request can take the first BEFORE its shadow march - one value crosses the march, as cosNL did, and the specular term's
// temporaries (and the sample's position) are dead by then.  shade_light: what the light contributes to an unshadowed sample, (kd * cosNL) * I2
// [+ (ks * sp) * I2]; shade_factor: ka + that * (1 - shadow).  The reference's state (0.5, 0.5, 0, -, I2 = 2) is its literal expression,
// 0.5f + 0.5f * cosNL * 2.f * (1.f - shadow) (shaders_raymarching.cu:156-157), operation for operation.  Material, light and camera are kernel
// arguments: scalar registers, and the specular term sits behind a wave-uniform branch on ks > 0.
// MAT = false is the reference state with its values as literals: the kernels every frame runs until a setter is called are the ones that existed
// before the setters did.  (One kernel for both was tried: nine more live scalars - the shade kernels spill scalars already - moved every
// shading instantiation, +3 ... +6 VGPRs and an occupancy step for the gradient-shaded quad layouts, +11 ... +18 spilled scalars with shadows;
// profiles/r08_lighting.md.)  The host picks MAT = true when the committed material or intensity is not the reference's (reference_material).
__host__ __device__ inline bool reference_material(const RayMarchParams& P) { return P.mat_ka == 0.5f && P.mat_kd == 0.5f && P.mat_ks == 0.f && P.light_i2 == 2.f; }
// ORTHO: the view vector of the orthographic camera, -cam_dir for every sample (no position enters)
template <bool MAT, bool ORTHO = false>
__device__ __forceinline__ float shade_light(const RayMarchParams& P, f3 light, f3 n_w, f3 pos)
{
  const float cosNL = fabsf(dot3(light, n_w));
  float d = ((MAT ? P.mat_kd : 0.5f) * cosNL) * (MAT ? P.light_i2 : 2.f);
  if (MAT && P.mat_ks > 0.f) {
    const f3 v = ORTHO ? mk3(-P.cam_dir.x, -P.cam_dir.y, -P.cam_dir.z)
                       : normalize3(mk3(P.cam_pos.x - pos.x, P.cam_pos.y - pos.y, P.cam_pos.z - pos.z)); // from the sample's position, not from its ray: a pooled request holds no direction
    const f3 h = normalize3(mk3(light.x + v.x, light.y + v.y, light.z + v.z));
    const float cosNH = fabsf(dot3(h, n_w)); // two-sided, like the diffuse term
    // NaN (a sample at the camera, h of length 0) and denormals (v_log_f32 takes them for 0: -inf, times shininess 0 = NaN) select 0
#if OVR_PARITY_EXACT
    const float pw = det_exp2f(P.mat_shininess * det_log2f(cosNH));
#else
    const float pw = __builtin_amdgcn_exp2f(P.mat_shininess * __builtin_amdgcn_logf(cosNH));
#endif
    const float sp = cosNH >= FLT_MIN ? pw : 0.f;
    d = d + (P.mat_ks * sp) * P.light_i2;
  }
  return d;
}
template <bool MAT>
__device__ __forceinline__ float shade_factor(const RayMarchParams& P, float lit, float shadow) { return (MAT ? P.mat_ka : 0.5f) + lit * (1.f - shadow); }

// The shadow cache's lookup (include/ovr_hip.h ovr_hip_set_shadow_cache; open-volume-renderer_amd/shadow_cache.py is the normative arithmetic): the shadow
// term of a sample at the object position po as one trilinear tap into the lattice of march_shadow's values - eight scalar loads and seven lerps, along x,
// then y, then z, whatever the voxel type, layout or addressing mode.  The lattice and its dimensions are kernel arguments behind every other one
// (RayMarchParams::shadow_lattice / shadow_n1): only the cached instantiations read them.  The result is not clamped.
__device__ __forceinline__ float shadow_lookup(const RayMarchParams& P, f3 po)
{
  const int nx1 = P.shadow_n1[0], ny1 = P.shadow_n1[1], nz1 = P.shadow_n1[2]; // N - 1 per axis (>= 1)
  const float gx = clamp01(po.x) * (float)nx1, gy = clamp01(po.y) * (float)ny1, gz = clamp01(po.z) * (float)nz1;
  const int ix = min((int)floorf(gx), nx1 - 1), iy = min((int)floorf(gy), ny1 - 1), iz = min((int)floorf(gz), nz1 - 1);
  const float fx = gx - (float)ix, fy = gy - (float)iy, fz = gz - (float)iz;
  const size_t sy = (size_t)nx1 + 1, sz = sy * ((size_t)ny1 + 1);
  const float* __restrict__ c = P.shadow_lattice + ((size_t)ix + sy * (size_t)iy + sz * (size_t)iz);
  const float v000 = c[0], v100 = c[1], v010 = c[sy], v110 = c[sy + 1], v001 = c[sz], v101 = c[sz + 1], v011 = c[sz + sy], v111 = c[sz + sy + 1];
  const float c00 = lerpf(v000, v100, fx), c10 = lerpf(v010, v110, fx), c01 = lerpf(v001, v101, fx), c11 = lerpf(v011, v111, fx);
  return lerpf(lerpf(c00, c10, fy), lerpf(c01, c11, fy), fz);
}

// shade one request: gradient (shaders_common.h:195-215), normals, shadow march, shade factor
// (shaders_raymarching.cu:124-158).  Writes the result over the request.
// CACHED: the shadow term is shadow_lookup's tap instead of a march (SHADE == 1: the kernel has no shadow march)
// ORTHO: the orthographic camera's view vector (shade_light)
template <int VT, int SHADE, int AM, bool SKIP, bool MAT, bool CLIP = false, bool CACHED = false, bool ORTHO = false>
__device__ __forceinline__ void shade_request(const RayMarchParams& P, const VolConsts& vc, const TfConsts& tf, const MarchConsts& mc, ShadeReq& r,
                                              unsigned int& n_shadow, unsigned int& n_shadow_skipped)
{
  const f3 pos = mk3(r.px, r.py, r.pz);
  const f3 po = to_object(mc, pos);
  // one-sided differences, flipped at the upper bound; the three taps are issued together
  const bool flx = (po.x + mc.gstep.x) > 1.f, fly = (po.y + mc.gstep.y) > 1.f, flz = (po.z + mc.gstep.z) > 1.f;
  const f3 pgx = mk3(po.x + (flx ? -mc.gstep.x : mc.gstep.x), po.y, po.z), pgy = mk3(po.x, po.y + (fly ? -mc.gstep.y : mc.gstep.y), po.z);
  const f3 pgz = mk3(po.x, po.y, po.z + (flz ? -mc.gstep.z : mc.gstep.z));
  Tap tgx, tgy, tgz;
  tap_issue<VT, AM>(vc, pgx, tgx);
  tap_issue<VT, AM>(vc, pgy, tgy);
  tap_issue<VT, AM>(vc, pgz, tgz);
  const f3 rgb = tf_color(tf, r.v);
  const float sgx = tap_finish<VT>(vc, tgx), sgy = tap_finish<VT>(vc, tgy), sgz = tap_finish<VT>(vc, tgz);
  f3 g;
#if OVR_PARITY_EXACT
  g.x = (sgx - r.s) / (flx ? -mc.gstep.x : mc.gstep.x); // (sample(c + stp) - v) / stp, shaders_common.h:195-215
  g.y = (sgy - r.s) / (fly ? -mc.gstep.y : mc.gstep.y);
  g.z = (sgz - r.s) / (flz ? -mc.gstep.z : mc.gstep.z);
#else
  g.x = (sgx - r.s) * (flx ? -mc.ginv.x : mc.ginv.x);
  g.y = (sgy - r.s) * (fly ? -mc.ginv.y : mc.ginv.y);
  g.z = (sgz - r.s) * (flz ? -mc.ginv.z : mc.ginv.z);
#endif
  const f3 gn = normalize3(g);
  const f3 n_o = mk3(-gn.x, -gn.y, -gn.z);
  const f3 n_w = normalize3(mk3(n_o.x * mc.otw_it.x, n_o.y * mc.otw_it.y, n_o.z * mc.otw_it.z));
  f3 n_c = mk3(0, 0, 0);
  if (P.grad) {
    const float* m = P.wtc_it;
    n_c = normalize3(mk3(fmaf(n_w.x, m[0], fmaf(n_w.y, m[3], n_w.z * m[6])), fmaf(n_w.x, m[1], fmaf(n_w.y, m[4], n_w.z * m[7])),
                         fmaf(n_w.x, m[2], fmaf(n_w.y, m[5], n_w.z * m[8]))));
  }
  const float lit = shade_light<MAT, ORTHO>(P, mc.light, n_w, pos);
  float shadow = 0.f;
  if (SHADE == 2) shadow = march_shadow<VT, AM, kShadowTaps, SKIP, CLIP>(P, vc, tf, mc, pos, n_shadow, n_shadow_skipped);
  if (CACHED) shadow = shadow_lookup(P, po);
  const float shade = shade_factor<MAT>(P, lit, shadow); // shaders_raymarching.cu:156-157
  const float tr = r.tr;
  r.px = tr * clamp01(rgb.x * shade);
  r.py = tr * clamp01(rgb.y * shade);
  r.pz = tr * clamp01(rgb.z * shade);
  r.s = tr * clamp01(n_c.x);
  r.v = tr * clamp01(n_c.y);
  r.tr = tr * clamp01(n_c.z);
}

// hand the contributions of one shaded batch (stream positions [base, base + n), result of position base + j in lane j)
// back to the owning lanes: every owner walks its own requests of this batch in sample order
__device__ __forceinline__ void apply_batch(const ShadeReq& res, unsigned int base, unsigned int n, int lane, int& pend, unsigned int& first, f3& color,
                                            f3& gradient)
{
  for (;;) {
    const bool has = (pend > 0) && ((first - base) < n);
    if (__ballot(has) == 0ull) break;
    const int j = has ? (int)(first - base) : lane;
    const float tcx = bperm(j, res.px), tcy = bperm(j, res.py), tcz = bperm(j, res.pz);
    const float tgx = bperm(j, res.s), tgy = bperm(j, res.v), tgz = bperm(j, res.tr);
    const float ta = bperm(j, res.a);
    const int tn = bperm_i(j, res.next);
    if (has) {
      color.x = fmaf(tcx, ta, color.x);
      color.y = fmaf(tcy, ta, color.y);
      color.z = fmaf(tcz, ta, color.z);
      gradient.x = fmaf(tgx, ta, gradient.x);
      gradient.y = fmaf(tgy, ta, gradient.y);
      gradient.z = fmaf(tgz, ta, gradient.z);
      first = (unsigned int)tn;
      --pend;
    }
  }
}

constexpr int kNC = kBlockCounters; // counters: rays, samples, shaded, shadow, active pixels, skipped samples, skipped shadow samples, hits through an ignored slab (ignored_slab_outside)
// per-wave counters -> LDS -> one plain store of the workgroup's partial sums (lds must hold kWaves*kNC uints)
__device__ __forceinline__ void store_block_counters(const RayMarchParams& P, unsigned int* red, int lane, int wave, unsigned int n_rays,
                                                     unsigned int n_samples, unsigned int n_shaded, unsigned int n_shadow, unsigned int n_active,
                                                     unsigned int n_skipped, unsigned int n_shadow_skipped, unsigned int n_outside_hits)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_rays += __shfl_down(n_rays, off);
    n_samples += __shfl_down(n_samples, off);
    n_shaded += __shfl_down(n_shaded, off);
    n_shadow += __shfl_down(n_shadow, off);
    n_active += __shfl_down(n_active, off);
    n_skipped += __shfl_down(n_skipped, off);
    n_shadow_skipped += __shfl_down(n_shadow_skipped, off);
    n_outside_hits += __shfl_down(n_outside_hits, off);
  }
  if (!P.block_counters) return;
  __syncthreads(); // LDS is dead at this point: reuse its front
  if (lane == 0) {
    red[wave * kNC + 0] = n_rays; red[wave * kNC + 1] = n_samples; red[wave * kNC + 2] = n_shaded;
    red[wave * kNC + 3] = n_shadow; red[wave * kNC + 4] = n_active; red[wave * kNC + 5] = n_skipped; red[wave * kNC + 6] = n_shadow_skipped;
    red[wave * kNC + 7] = n_outside_hits;
  }
  __syncthreads();
  if (threadIdx.x < kNC) {
    const unsigned int bid = blockIdx.x;
    unsigned int sum = 0;
    for (int w = 0; w < kWaves; ++w) sum += red[w * kNC + threadIdx.x];
    P.block_counters[(size_t)bid * kNC + threadIdx.x] = sum;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// the march kernel (both pipelines)
//
// Lane mapping - "four lanes per ray": a wave handles 16 rays (a 4x4 pixel tile); the 4 lanes of a quad are 4 CONSECUTIVE
// STEPS of one ray.  The texture addresser coalesces a gather only inside quads of 4 consecutive lanes (16 clocks per
// instruction when a quad shares a 128-byte line, 66 when its lanes hit 4 lines - tools/ubench_lines.hip); with one lane
// per pixel (2 voxels apart at the bench's resolution) a quad almost never shared a brick, with 4 lanes per ray its taps
// are 1 voxel apart and nearly always do.  A round = K instructions x 4 steps; every lane recomputes the ray's t sequence
// (tx, ty recurrence, shaders_raymarching.cu:168-169) and the alpha recurrence (:165) for all 4K steps, fetching the
// other lanes' opacities with DPP quad broadcasts, so the arithmetic and its order are exactly the reference's.
//   POOLED = false: shade queued requests in place (raymarch pipeline 1)      POOLED = true: spill them to the pool
// ------------------------------------------------------------------------------------------------------------------
template <int B>
__device__ __forceinline__ float quad_bcast(float x) // value of lane B of this lane's quad
{
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), B * 0x55, 0xf, 0xf, true));
}
// a_sub for the lane's sub = lane & 3.  As nested conditionals the compiler builds this from compares and exec-mask branches (5 vector + 7
// scalar instructions per select, 8 selects per round of the march); with the two lane masks m1 = -(sub & 1), m2 = -((sub >> 1) & 1) kept in
// registers it is three v_bfi_b32 (bit-field insert: (m & b) | (~m & a)) - the same bits
struct SubMask { unsigned int m1, m2; int sub; };
__device__ __forceinline__ SubMask make_submask(int sub) { SubMask m; m.m1 = 0u - (unsigned int)(sub & 1); m.m2 = 0u - (unsigned int)((sub >> 1) & 1); m.sub = sub; return m; }
__device__ __forceinline__ unsigned int bfi(unsigned int m, unsigned int b, unsigned int a) { return (m & b) | (~m & a); }
__device__ __forceinline__ float sel4(float a0, float a1, float a2, float a3, const SubMask& m)
{
  const unsigned int lo = bfi(m.m1, __float_as_uint(a1), __float_as_uint(a0)), hi = bfi(m.m1, __float_as_uint(a3), __float_as_uint(a2));
  return __uint_as_float(bfi(m.m2, hi, lo));
}

// Blue-noise pixel jitter (P.jitter_mode == 1; BASELINE C5, north_star): sample k of frame f takes slice
// t = ((f - 1) * spp + k) % 64 of the noise tile (lookup as blue_noise.h:95-99; the tile is stored transposed, [t][y][x]):
// xi0 = tile[t][iy % xy][ix % xy], xi1 = the same slice shifted by half a tile in x and y.  In dense mode the workgroup
// stages the 2 x 64 variates of its 8x8 pixels for the first kJitStaged samples in LDS; later samples and sparse-mode
// pixels read the tile directly.
constexpr int kJitStaged = 4;
__device__ __forceinline__ int jitter_slice(const RayMarchParams& P, int k) { return (int)((((long long)P.frame_index - 1) * P.spp + k) % 64); }
__device__ __forceinline__ void jitter_global(const RayMarchParams& P, int ix, int iy, int k, float& x0, float& x1)
{
  const int xy = P.jitter_xy, h = xy >> 1;
  const float* slice = P.jitter_noise + (size_t)jitter_slice(P, k) * xy * xy;
  x0 = slice[(size_t)(iy % xy) * xy + (ix % xy)];
  x1 = slice[(size_t)((iy + h) % xy) * xy + ((ix + h) % xy)];
}

// which pixel does this QUAD own?  (4x4 pixels per wave, 8x8 per workgroup; sparse mode: 64 list entries per workgroup)
// Dense mode: workgroup s of the 1-D grid renders the 8x8 block P.schedule[s] = bx | by << 16 - the blocks this rank owns,
// longest rays first (launch_schedule) - compute_screen_position of the reference (shaders_common.h:394-451) is the
// identity on the launch index, which fixes neither an order nor a grouping.
__device__ __forceinline__ bool assign_pixel_quad(const RayMarchParams& P, int lane, int wave, int& ix, int& iy)
{
  const int ray = lane >> 2;
  bool active;
  if (P.sparse_xy) {
    const unsigned long long i = (unsigned long long)blockIdx.x * (kBlock / 4) + (unsigned int)(threadIdx.x >> 2);
    active = (2ull * i) < *P.sparse_count;
    ix = active ? P.sparse_xy[2 * i] : 0;
    iy = active ? P.sparse_xy[2 * i + 1] : 0;
  }
  else {
    const unsigned int e = P.schedule[blockIdx.x];
    ix = (int)(e & 0xffffu) * 8 + (wave & 1) * 4 + (ray & 3);
    iy = (int)(e >> 16) * 8 + (wave >> 1) * 4 + (ray >> 2);
    active = ix < P.width && iy < P.height;
  }
  if (P.world > 1 && active) active = ((ix / P.tile_w + iy / P.tile_h) % P.world) == P.rank;
  return active;
}

// the primary rays' form: the 4 lanes of the quad each walk a quarter of [t0, t1]; min / max over the quad.  Two levels: the
// coarse grid over the whole ray, then - only inside the coarse interval - the per-macrocell grid: a primary ray is long (its
// coarse interval is up to 80 voxels too wide at either end, and a ray that only grazes the dilated coarse entries gets an
// interval although it meets nothing), and every round inside the interval costs ~330 instead of ~45 instructions.
template <bool FINE>
__device__ __forceinline__ void skip_interval_level(const VolConsts& vc, f3 oo, f3 od, float t0, float t1, int sub, bool live, float& t_first, float& t_last)
{
  float first = FLT_MAX, last = -FLT_MAX;
  if (live) {
    const float len = t1 - t0;
    const float ta = fmaf((float)sub * 0.25f, len, t0), tb = sub == 3 ? t1 : fmaf((float)(sub + 1) * 0.25f, len, t0);
    skip_walk<FINE>(vc, oo, od, ta, tb, first, last);
  }
  t_first = fminf(fminf(quad_bcast<0>(first), quad_bcast<1>(first)), fminf(quad_bcast<2>(first), quad_bcast<3>(first)));
  t_last = fmaxf(fmaxf(quad_bcast<0>(last), quad_bcast<1>(last)), fmaxf(quad_bcast<2>(last), quad_bcast<3>(last)));
}
__device__ __forceinline__ SkipSpan skip_interval(const VolConsts& vc, f3 oo, f3 od, float t0, float t1, int sub, bool live)
{
  SkipSpan sp = skipspan_none();
  sp.mask_lo = sp.mask_hi = ~0u;
  skip_interval_level<false>(vc, oo, od, t0, t1, sub, live, sp.first, sp.last);
  const float c0 = sp.first, c1 = sp.last; // quad-uniform
  const bool walk = live && c0 <= c1;
  if (__ballot(walk) != 0ull) skip_interval_level<true>(vc, oo, od, c0, c1, sub, walk, sp.first, sp.last);
  return sp;
}

// Register budget: at most 3 waves per SIMD (up to 168 VGPRs).  Left alone the compiler squeezes the kernel into 128 VGPRs
// for a 4th wave by serialising the K tap groups it is supposed to keep in flight - measured 1.98 instead of 1.53 ms on C3.
constexpr int kMarchWavesPerEu = 3;
// LDSB = true: the "LDS-staged bricks" variant (north_star; measured in profiles/r02_notes.md).  Once per round the workgroup
// copies the bricks its 64 rays touch in the round's 16 steps - the brick-aligned bounding box of the block's four corner
// rays over the round's t range - from HBM / L2 into LDS with whole-line 16-byte loads (8 lanes per 128-byte brick), and the
// round's taps read LDS (ds_read2_b32 pairs) instead of going through the texture addresser.  A round whose box exceeds the LDS
// budget, and a tap that falls outside the staged box, take the ordinary path - the result is bit-identical either way.
// Built for the in-place, unshaded march of the general f32 layout (BASELINE C2, where rays are denser than voxels).
// (kLdsBrickCap bricks per workgroup, QCfg: host/launch_plan.hpp)
struct LdsRegion { int bx0, by0, bz0, ebx, eby, ebz, nbr, ok; };
static_assert(sizeof(LdsRegion) == kLdsRegionBytes, "launch_plan.hpp restates the region descriptor's size");
// DEEP = true (plain pooled march only): 6 instead of 4 instructions (x 4 steps) per round - 24 pair loads in flight per lane at 2
// waves per SIMD (198 VGPRs) instead of 16 at 3.  On a full frame the two are within 1 % of each other (and 4 is better with dense
// transfer functions and on axis views), but a ray's chain of dependent rounds is the floor of an image SHARD's march, and there 6
// wins: 8-way shard of C3 0.295 -> 0.250 ms, 4-way 0.451 -> 0.423 (profiles/r02_notes.md).  plan_launch picks it for small shards (deep_rounds_pay).
constexpr int kDeepK = 6;
// (the skipping pooled march sits at the edge of the 3-waves budget: 169 VGPRs - one too many - cost it 15 %; it is pinned to 3)
constexpr int kPinMaxAM = 1; // the 64-bit addressing modes would spill to scratch under the pin
// CLIP = true: the clipped march (box_test).  Where the march shades in place it rides on MAT = true - the material's values as arguments give the
// reference state's bits when they are the reference's - so a clipped state adds one instantiation per kernel, not two
// CACHED = true: the shadow cache's frame (shade_request) - SHADE == 1 and MAT = true, in place only
// ORTHO = true: the orthographic camera (pixel_ray: a per-lane origin; primary_box_test; shade_light's view vector) - on the clipped variants alone, never
// LDS-staged or deep
template <int VT, int SHADE, int AM, bool POOLED, bool SKIP, bool LDSB = false, bool DEEP = false, bool MAT = false, bool CLIP = false, bool CACHED = false,
          bool ORTHO = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu((SKIP && POOLED && (AM == 4 ? 0 : AM) <= kPinMaxAM) ? kMarchWavesPerEu : 1, kMarchWavesPerEu))) void raymarch_kernel(const RayMarchParams P)
{
  static_assert(march_variant_exists(SHADE, AM, POOLED, SKIP, LDSB, DEEP, MAT, CLIP, VT == VOX_F32, CACHED, ORTHO), "no such variant of the march (host/launch_plan.hpp)");
  using Cfg = QCfg<SHADE, POOLED>;
  constexpr int K = DEEP ? kDeepK : Cfg::K;
  constexpr int QCAP = Cfg::QCAP;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & 3;               // this lane's step inside each group of 4 consecutive steps
  const int qbase = lane & ~3;            // first lane of the quad
  const bool owner = sub == 0;            // the quad's lane that keeps the pixel's colour / request list
  const SubMask subm = make_submask(sub);
  const unsigned long long t_start = P.trace ? __builtin_amdgcn_s_memrealtime() : 0ull;

  int ix, iy;
  const bool active = assign_pixel_quad(P, lane, wave, ix, iy);
  unsigned int n_rays = 0, n_samples = 0, n_shaded = 0, n_shadow = 0, n_skipped = 0, n_shadow_skipped = 0, n_outside_hits = 0;
  VolConsts vc;
  MarchConsts mc;
  setup_consts(P, vc, mc);

  // ---- LDS carve: [request queues][offset tables][TF colour (not needed by the pooled march)][TF alpha]
  // A workgroup none of whose rays can hit the volume (most of the image outside the silhouette) stages nothing; with
  // empty-space skipping, neither does one whose rays only cross empty macrocells.
  ShadeReq* const queue = reinterpret_cast<ShadeReq*>(lds_raw) + (size_t)wave * (QCAP > 0 ? QCAP : 1);
  TfConsts tf;
  SkipSpan pro_span = skipspan_none(); // skipping, spp == 1: the ray's skip hull and segment mask, found here once
  const float rsx = 1.f / (float)P.width, rsy = 1.f / (float)P.height;
  const float scx = ((float)ix + .5f) * rsx, scy = ((float)iy + .5f) * rsy;
  // pooled: one launch per sample-per-pixel generation (P.spp_index), in place: all here.  min(P.spp, 1) is 1, but as a
  // run-time value: with a constant trip count of 1 the compiler restructures the kernel into a schedule that keeps fewer
  // taps in flight (126 instead of 153 VGPRs) and the C3 march takes 1.98 instead of 1.53 ms
  const int spp = POOLED ? min(P.spp, 1) : P.spp;
  // blue-noise jitter: the variates of this block's pixels, staged in LDS (dense mode) for the samples this launch renders
  __shared__ float jit_lds[kJitStaged][2][64];
  const bool jit_staged = P.jitter_mode == 1 && !P.sparse_xy;
  if (jit_staged) {
    const unsigned int e = P.schedule[blockIdx.x];
    const int xy = P.jitter_xy, h = xy >> 1;
    const int nk = min(spp, kJitStaged);
    for (int i = threadIdx.x; i < nk * 128; i += kBlock) {
      const int k = i >> 7, d = (i >> 6) & 1, p = i & 63;
      const int px = (int)(e & 0xffffu) * 8 + (p & 7) + d * h, py = (int)(e >> 16) * 8 + (p >> 3) + d * h;
      jit_lds[k][d][p] = P.jitter_noise[(size_t)jitter_slice(P, (POOLED ? P.spp_index : 0) + k) * xy * xy + (size_t)(py % xy) * xy + (px % xy)];
    }
    __syncthreads();
  }
  // the two jitter variates of sample k (k counts the samples of this launch)
  auto jitter = [&](int k, float& x0, float& x1) {
    if (jit_staged && k < kJitStaged) {
      const int ray = lane >> 2;
      const int p = ((wave >> 1) * 4 + (ray >> 2)) * 8 + (wave & 1) * 4 + (ray & 3);
      x0 = jit_lds[k][0][p];
      x1 = jit_lds[k][1][p];
    }
    else jitter_global(P, ix, iy, (POOLED ? P.spp_index : 0) + k, x0, x1);
  };
  bool staged; // workgroup-uniform: the offset tables and the transfer function are in LDS
  {
    bool need = active;
    if (P.spp == 1 && active) { // spp == 1: the ray is known - test it (the same expressions as the march below uses)
      float sx0 = scx, sy0 = scy;
      if (P.jitter_mode == 1) {
        float j0, j1;
        jitter(0, j0, j1);
        sx0 += (j0 - 0.5f) * rsx;
        sy0 += (j1 - 0.5f) * rsy;
      }
      const float ux0 = sx0 - 0.5f, uy0 = sy0 - 0.5f;
      f3 o0, d0;
      pixel_ray<ORTHO>(P, ux0, uy0, o0, d0);
      float a0 = 0.f, b0 = FLT_MAX;
      const f3 oo0 = to_object(mc, o0), od0 = mk3(d0.x * mc.inv_scale.x, d0.y * mc.inv_scale.y, d0.z * mc.inv_scale.z);
      need = primary_box_test<CLIP, ORTHO>(P, a0, b0, oo0, od0);
      if (SKIP && need) { // skipping: a ray that meets no occupied macrocell never fetches a voxel or a TF entry either
        pro_span = skip_interval(vc, oo0, od0, a0, b0, sub, true);
        need = pro_span.first <= pro_span.last;
      }
    }
    staged = __syncthreads_or(need ? 1 : 0) != 0;
    if (staged) {
      unsigned char* base = lds_raw + (size_t)kWaves * QCAP * sizeof(ShadeReq);
      const size_t tb = (stage_tables<VT, AM>(P, base, vc) + 15) & ~(size_t)15;
      stage_tf(P, base + tb, !POOLED, tf);
    }
    else {
      tf = TfConsts{};
      vc.tab_x = vc.tab_y = vc.tab_z = nullptr;
      vc.tab_z64 = nullptr;
    }
  }
  const PoolDesc& Q = P.pool;
  const unsigned int tile = blockIdx.x * kWaves + wave;
  // LDS-staged bricks: [.. tables, TF ..][bricks: kLdsBrickCap x 128 B][region descriptor][corner rays 4 x float3][t range]
  float* const lds_bricks = LDSB ? reinterpret_cast<float*>(lds_raw + P.lds_brick_offset) : nullptr;
  LdsRegion* const lds_region = reinterpret_cast<LdsRegion*>(lds_bricks + (size_t)kLdsBrickCap * 32);
  float* const lds_corner = reinterpret_cast<float*>(lds_region + 1);
  int* const lds_trange = reinterpret_cast<int*>(lds_corner + 12);
  unsigned int n_lds_fb_taps = 0, n_lds_fb_rounds = 0; // diagnostics: taps outside the staged box, rounds whose box did not fit
  if (LDSB && threadIdx.x < 4) { // directions of the block's corner rays, half a pixel outside the corner pixels (covers any jitter)
    const unsigned int e = P.schedule[blockIdx.x];
    const float cx_ = ((float)((int)(e & 0xffffu) * 8 + ((threadIdx.x & 1) ? 8 : 0))) / (float)P.width - 0.5f;
    const float cy_ = ((float)((int)(e >> 16) * 8 + ((threadIdx.x & 2) ? 8 : 0))) / (float)P.height - 0.5f;
    f3 o_, d; // (LDS staging is the perspective camera's alone: one origin, P.cam_pos, for the whole block)
    pixel_ray<false>(P, cx_, cy_, o_, d);
    lds_corner[3 * threadIdx.x] = d.x; lds_corner[3 * threadIdx.x + 1] = d.y; lds_corner[3 * threadIdx.x + 2] = d.z;
  }

  const unsigned int pixel_index = (unsigned int)ix + (unsigned int)iy * (unsigned int)P.width;
  unsigned int v0 = (unsigned int)P.frame_index, v1 = pixel_index; // RandomTEA(frame_index, pixel_index)
  // the perspective camera's origin is the frame's: wave-uniform, formed once; the orthographic camera's is the sample's (pixel_ray, below)
  f3 org = ld3(P.cam_pos);
  f3 oo = to_object(mc, org);

  float o_a = 0.f;
  f3 o_c = mk3(0, 0, 0), o_g = mk3(0, 0, 0);
  if (POOLED && P.spp > 1)
    for (int i = 0; i < P.spp_index; ++i) tea16(v0, v1); // RandomTEA state of this generation (random.h:146-188)
  // wave-uniform queue cursors (stream positions; slot = position & (QCAP - 1))
  unsigned int q_head = 0, q_tail = 0;
  // pooled: the tile's current reservation of consecutive chunks - kRun at first, doubling up to kRunMax with every further
  // reservation: a tile that pushes a lot (dense transfer function: every sample is shaded) would otherwise hit the one
  // pool counter every round - 48 k same-address returning atomics per C3 frame, which serialise in L2
  unsigned int run_base = 0, run_left = 0, run_size = 0, run_next = kRun;
  bool run_ok = true; // the current reservation lies inside its sub-pool
  int prev_chunk = -1;
  if (POOLED && lane == 0) Q.tile_first[tile] = -1;
  // per-ray request list (identical in the 4 lanes of the quad; the owner lane applies the contributions)
  int pend = 0;
  unsigned int first = 0, last = 0, last_gidx = 0;
  float alpha = 0.f;
  f3 color = mk3(0, 0, 0), gradient = mk3(0, 0, 0);

  // pooled: spill the n oldest queued requests as one chunk of the global pool
  auto spill = [&](unsigned int n) {
    if (run_left == 0) {
      const unsigned int sub = blockIdx.x & (unsigned int)(kPoolSubs - 1); // the workgroup's sub-pool (PoolDesc)
      unsigned int c0 = 0;
      if (lane == 0) c0 = atomicAdd(&Q.ctrl[32u * (sub + 1u)], run_next);
      c0 = (unsigned int)__builtin_amdgcn_readfirstlane((int)c0);
      run_left = run_size = run_next;
      run_ok = c0 + run_size <= Q.sub_capacity;
      if (!run_ok && lane == 0) Q.ctrl[1] = 1u; // the counter keeps counting: the host sees how much was asked for
      run_base = sub * Q.sub_capacity + c0;
      run_next = min(run_next * 2u, (unsigned int)kRunMax);
    }
    const unsigned int c = run_base + (run_size - run_left);
    --run_left;
    if (run_ok) {
      __builtin_amdgcn_wave_barrier();
      if ((unsigned int)lane < n) Q.reqs[(size_t)c * 64 + lane] = queue[(q_head + lane) & (QCAP - 1)];
      if (lane == 0) {
        Q.chunk_n[c] = n;
        if (prev_chunk >= 0) Q.chunk_next[prev_chunk] = (int)c; else Q.tile_first[tile] = (int)c;
        if (Q.order && (c & (unsigned int)(kRun - 1)) == 0u) { // the first chunk of a run: its beam (shade order, PoolDesc)
          const ShadeReq& r0 = queue[q_head & (QCAP - 1)];
          const unsigned int key = beam_index(Q, r0.px, r0.py, r0.pz);
          Q.order_key[c / (unsigned int)kRun] = key;
          atomicAdd(&Q.order_ws[kOrderHist + key], 1u);
        }
      }
      if (pend > 0 && (last - q_head) < n) last_gidx = c * 64u + (last - q_head);
      prev_chunk = (int)c;
    }
    // beyond the sub-pool: it is exhausted; its counter keeps counting so the host knows how much was needed, re-sizes
    // the pool and renders the frame again (ovr_hip_api.cpp) - nothing of this frame is used
    q_head += n;
  };

  for (int k_spp = 0; k_spp < spp; ++k_spp) { // uniform trip count: every lane of the wave runs every round
    float sx = scx, sy = scy;
    if (P.jitter_mode == 1) {
      float j0, j1;
      jitter(k_spp, j0, j1);
      sx += (j0 - 0.5f) * rsx;
      sy += (j1 - 0.5f) * rsy;
    }
    else if (P.spp > 1) {
      tea16(v0, v1);
      sx += ((float)v0 * OVR_TEA_TOFLOAT - 0.5f) * rsx;
      sy += ((float)v1 * OVR_TEA_TOFLOAT - 0.5f) * rsy;
    }
    const float ux = sx - 0.5f, uy = sy - 0.5f;
    f3 dir;
    if (ORTHO) { pixel_ray<true>(P, ux, uy, org, dir); oo = to_object(mc, org); }
    else { f3 o_; pixel_ray<false>(P, ux, uy, o_, dir); }
    // ---- __intersection__volume: object-space ray, direction not renormalised so t is shared
    const f3 od = mk3(dir.x * mc.inv_scale.x, dir.y * mc.inv_scale.y, dir.z * mc.inv_scale.z);
    float t0 = 0.f, t1 = FLT_MAX;
    alpha = 0.f;
    color = mk3(0, 0, 0);
    gradient = mk3(0, 0, 0);
    bool live = active && primary_box_test<CLIP, ORTHO>(P, t0, t1, oo, od);
    if (active && owner) ++n_rays;
    if (live && owner && box_ignored_slab_outside<CLIP>(P, oo, od)) ++n_outside_hits;
    SkipSpan span = skipspan_all(); // samples outside the hull, or in an unmarked segment of it, are in empty macrocells
    if (SKIP) {
      if (P.spp == 1) span = pro_span; // same ray, same [t0, t1] as in the prologue
      else span = skip_interval(vc, oo, od, t0, t1, sub, live);
    }
    // `staged` guards the prologue's decision (it tests the same ray with the same expressions): without the tables and the TF
    // in LDS no sample may be fetched - a skipping ray then only counts its (all empty) steps, any other ray is dead
    if (SKIP) { if (!staged) span = skipspan_none(); }
    else live = live && staged;
    float tx = t0, ty = fminf(t1, t0 + mc.step);
    pend = 0;
    unsigned int lds_round = 0;
    if (LDSB) { // the workgroup's range of entry distances: round r of every ray lies in [tmin + 16 r step, tmax + 16 (r + 1) step]
      __syncthreads();
      if (threadIdx.x == 0) { lds_trange[0] = 0x7f7fffff; lds_trange[1] = 0; }
      __syncthreads();
      if (live) { atomicMin(&lds_trange[0], __float_as_int(t0)); atomicMax(&lds_trange[1], __float_as_int(t0)); } // t0 >= 0: ordered as ints
      __syncthreads();
    }

    for (;;) {
      // LDSB: the rounds are workgroup-synchronous (the staging below has barriers): all four waves run until no ray of the block is live
      const bool any_live = LDSB ? (__syncthreads_or(live ? 1 : 0) != 0) : (__ballot(live) != 0ull);
      // ---- (1) in place: shade queued requests, a full batch whenever 64 are queued, the remainder once no ray is live
      if (SHADE != 0 && !POOLED) {
        while ((q_tail - q_head) >= 64u || (!any_live && q_tail != q_head)) {
          const unsigned int n = min(q_tail - q_head, 64u);
          __builtin_amdgcn_wave_barrier(); // requests were written by other lanes of this wave (LDS ops are in order)
          ShadeReq r;
          r.px = r.py = r.pz = r.s = r.v = r.tr = r.a = 0.f; r.next = 0;
          if ((unsigned int)lane < n) {
            r = queue[(q_head + lane) & (QCAP - 1)];
            if (r.a > 0.f) shade_request<VT, SHADE, AM, SKIP, MAT, CLIP, CACHED, ORTHO>(P, vc, tf, mc, r, n_shadow, n_shadow_skipped); // a == 0: null request
          }
          int opend = owner ? pend : 0;
          apply_batch(r, q_head, n, lane, opend, first, color, gradient);
          // the quad's lanes keep identical list cursors: take the owner's
          pend = __builtin_amdgcn_ds_bpermute(qbase << 2, opend);
          first = (unsigned int)__builtin_amdgcn_ds_bpermute(qbase << 2, (int)first);
          q_head += n;
        }
      }
      if (!any_live) break;

      // ---- (1b) empty-space skipping, bulk form: a round whose 4K steps all lie before (after) the ray's skip interval
      //      needs neither the lanes' own sample positions nor per-step bookkeeping - only the (tx, ty) recurrence, which
      //      has to be run step by step (its rounding is part of the result), and one validity test: the steps' midpoints
      //      lie in [tx_0, tx_4K], and validity (ty > tx) is monotone, so the last step being valid makes all of them valid.
      //      ~45 instructions per round instead of ~330 for the per-step form below.
      if (SKIP) {
        float ntx = tx, nty = ty, ptx = tx;
#pragma unroll
        for (int b = 0; b < 4 * K; ++b) {
          ptx = ntx;
          ntx = nty;
          nty = fminf(ntx + mc.step, t1);
        }
        const bool all_valid = ntx > ptx;                       // the round's last step: ty_last (= ntx) > tx_last (= ptx)
        const bool outside = !skipspan_touches(span, tx, ntx);
        const bool go = live && (alpha < 0.9999f);
        if (__ballot(live && !(outside && all_valid)) == 0ull) {
          n_skipped += go ? (unsigned int)K : 0u;               // this lane's K steps of the round
          live = go;
          tx = ntx; ty = nty;
          continue;
        }
      }
      // ---- (2) the ray's next 4K steps: every lane runs the (tx, ty) recurrence, keeps its own K steps and one validity
      //      bit per step (ty > tx, the first half of the reference's loop condition)
      unsigned int vmask = 0;
      Tap taps[K];
      f3 poss[K];
      float dts[K], mj[K], tms[K];
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
      }
      // empty-space fast path (wave-uniform): every sample of this round lies in a macrocell whose majorant is 0, so all
      // opacities are exactly 0, alpha does not move and nothing is pushed - only liveness and the counters advance
      auto skip_round = [&]() {
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            live = live && ((vmask >> (4 * k + b)) & 1u) != 0u && (alpha < 0.9999f);
            n_skipped += (live && sub == b) ? 1u : 0u;
          }
        }
      };
      if (SKIP) {
        // (a) by the ray's skip interval: no coordinates, no majorant lookups
        bool inside = false;
#pragma unroll
        for (int k = 0; k < K; ++k) inside = inside || skipspan_inside(span, tms[k]);
        if (__ballot(inside && live) == 0ull) { skip_round(); continue; }
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        poss[k] = mk3(fmaf(tms[k], dir.x, org.x), fmaf(tms[k], dir.y, org.y), fmaf(tms[k], dir.z, org.z));
        tap_coords(vc, to_object(mc, poss[k]), taps[k]);
        mj[k] = SKIP ? vc.majorant[tap_cell(vc, taps[k])] : 1.f; // empty-space skipping: the macrocell's max TF opacity
      }
      if (SKIP) {
        // (b) by the majorants of this round's own macrocells
        bool any = false;
#pragma unroll
        for (int k = 0; k < K; ++k) any = any || (mj[k] > 0.f);
        if (__ballot(any && live) == 0ull) { skip_round(); continue; }
      }
      if (LDSB) {
        typedef BrickMap<VT> M;
        // (a) wave 0: the brick-aligned box of this round - 4 corner rays x {t_lo, t_hi} (the rays of the block and the round's
        //     t range span a convex set between them), one voxel of margin, one more for the taps' upper neighbours
        if (wave == 0) {
          // (no safety margins: a tap that falls outside the box is caught below and read the ordinary way)
          const float t_lo = __int_as_float(lds_trange[0]) + (float)(lds_round * (unsigned)(4 * K)) * mc.step;
          const float t_hi = __int_as_float(lds_trange[1]) + (float)((lds_round + 1u) * (unsigned)(4 * K)) * mc.step;
          const int c = lane & 3;
          const float tt = (lane & 4) ? t_hi : t_lo;
          const f3 pw = mk3(fmaf(tt, lds_corner[3 * c], org.x), fmaf(tt, lds_corner[3 * c + 1], org.y), fmaf(tt, lds_corner[3 * c + 2], org.z));
          const f3 po = to_object(mc, pw);
          float lo[3] = { fmaf(po.x, vc.cs.x, vc.cb.x), fmaf(po.y, vc.cs.y, vc.cb.y), fmaf(po.z, vc.cs.z, vc.cb.z) };
          float hi[3] = { lo[0], lo[1], lo[2] };
#pragma unroll
          for (int off = 1; off < 8; off <<= 1)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              lo[a] = fminf(lo[a], __shfl_xor(lo[a], off));
              hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
            }
          if (lane == 0) {
            const int n1[3] = { vc.nx1, vc.ny1, vc.nz1 };
            int l[3], h[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              l[a] = min(max((int)floorf(fminf(fmaxf(lo[a], -4.f), 1e9f)), 0), n1[a]);
              h[a] = min(max((int)floorf(fminf(fmaxf(hi[a], -4.f), 1e9f)) + 1, 0), n1[a]); // + 1: the taps' upper neighbours
            }
            // along x the bricks are addressed by STORED position (voxel + 1): the pairs' lower members span [floor(lo) + 1, floor(hi) + 1]
            const int lu = min(max((int)floorf(fminf(fmaxf(lo[0], -4.f), 1e9f)) + 1, 0), n1[0] + 1);
            const int hu = min(max((int)floorf(fminf(fmaxf(hi[0], -4.f), 1e9f)) + 1, 0), n1[0] + 1);
            LdsRegion g;
            g.bx0 = (int)M::div_cx((unsigned)lu); g.by0 = l[1] >> Vox<VT>::by; g.bz0 = l[2] >> Vox<VT>::bz;
            g.ebx = (int)M::div_cx((unsigned)hu) - g.bx0 + 1; g.eby = (h[1] >> Vox<VT>::by) - g.by0 + 1; g.ebz = (h[2] >> Vox<VT>::bz) - g.bz0 + 1;
            g.nbr = g.ebx * g.eby * g.ebz;
            g.ok = g.nbr <= kLdsBrickCap ? 1 : 0;
            *lds_region = g;
          }
        }
        __syncthreads(); // also: every wave has finished reading the previous round's bricks
        const LdsRegion g = *lds_region;
        ++lds_round;
        n_shadow += (lane == 0 && wave == 0) ? 1u : 0u; // diagnostics: workgroup rounds (the unshaded march has no shadow samples)
        if (g.ok) {
          // (b) copy the bricks: 8 lanes x 16 bytes per brick, whole 128-byte lines.  (Issuing all of a thread's up to 12 loads
          //     into a register array before the first store was measured slower: 1.48 instead of 1.02 ms on C2 front.)
          const int row = threadIdx.x & 7;
          const float rcp_x = 1.f / (float)g.ebx, rcp_xy = 1.f / (float)(g.ebx * g.eby);
          for (int i = threadIdx.x >> 3; i < g.nbr; i += kBlock / 8) {
            const int iz = (int)(((float)i + 0.5f) * rcp_xy), rem = i - iz * g.ebx * g.eby;
            const int iy = (int)(((float)rem + 0.5f) * rcp_x), ixb = rem - iy * g.ebx;
            // (tab_x is indexed by voxel = stored position - 1; tab_y / tab_z by voxel)
            const unsigned int off = vc.tab_x[(g.bx0 + ixb) * Vox<VT>::cx - 1] + vc.tab_y[(g.by0 + iy) << Vox<VT>::by] + vc.tab_z[(g.bz0 + iz) << Vox<VT>::bz];
            const float4 v = AM == 0 ? *reinterpret_cast<const float4*>(static_cast<const char*>(vc.data) + off + row * 16)
                                     : *reinterpret_cast<const float4*>(static_cast<const float*>(vc.data) + off + row * 4);
            reinterpret_cast<float4*>(lds_bricks)[i * 8 + row] = v;
          }
          __syncthreads();
          // (c) the taps: region-relative brick index + position inside the brick; anything outside the box goes the ordinary way
          const int sxy = g.ebx * g.eby;
#pragma unroll
          for (int k = 0; k < K; ++k) {
            Tap& t = taps[k];
            const int y0 = max(t.y0, 0), z0 = max(t.z0, 0); // clamp-to-edge: index -1 reads voxel 0
            const int y1 = min(t.y0 + 1, vc.ny1), z1 = min(t.z0 + 1, vc.nz1);
            const int xu = t.x0 + 1;                          // stored position of the pair's lower member
            const int bxr = (int)M::div_cx((unsigned)xu), xr = xu - bxr * Vox<VT>::cx;
            const int cy0 = (y0 >> Vox<VT>::by) - g.by0, cy1 = (y1 >> Vox<VT>::by) - g.by0, cz0 = (z0 >> Vox<VT>::bz) - g.bz0, cz1 = (z1 >> Vox<VT>::bz) - g.bz0;
            const int cxr = bxr - g.bx0;
            const bool inside = (unsigned)cxr < (unsigned)g.ebx && (unsigned)cy0 < (unsigned)g.eby && (unsigned)cy1 < (unsigned)g.eby &&
                                (unsigned)cz0 < (unsigned)g.ebz && (unsigned)cz1 < (unsigned)g.ebz;
            if (inside) {
              constexpr int ym = (1 << Vox<VT>::by) - 1, zm = (1 << Vox<VT>::bz) - 1, SX = (int)M::SX;
              const int ox = cxr * (int)M::BV + xr;
              const int oy0 = cy0 * g.ebx * (int)M::BV + (y0 & ym) * SX, oy1 = cy1 * g.ebx * (int)M::BV + (y1 & ym) * SX;
              const int oz0 = cz0 * sxy * (int)M::BV + ((z0 & zm) << Vox<VT>::by) * SX, oz1 = cz1 * sxy * (int)M::BV + ((z1 & zm) << Vox<VT>::by) * SX;
              const float* b0 = lds_bricks + ox + oz0;
              const float* b1 = lds_bricks + ox + oz1;
              t.c000 = b0[oy0]; t.c100 = b0[oy0 + 1]; t.c010 = b0[oy1]; t.c110 = b0[oy1 + 1];
              t.c001 = b1[oy0]; t.c101 = b1[oy0 + 1]; t.c011 = b1[oy1]; t.c111 = b1[oy1 + 1];
            }
            else {
              tap_loads<VT, AM>(vc, t);
              n_lds_fb_taps += live ? 1u : 0u;
            }
          }
        }
        else {
          n_lds_fb_rounds += (lane == 0 && wave == 0) ? 1u : 0u;
#pragma unroll
          for (int k = 0; k < K; ++k) tap_loads<VT, AM>(vc, taps[k]);
        }
      }
      else {
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (!SKIP || mj[k] > 0.f) tap_loads<VT, AM>(vc, taps[k]);
      }
      // ---- (3) own samples: value, TF coordinate, corrected opacity (and colour when shading is off)
      float sa[K], va[K], aa[K];
      f3 ca[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        sa[k] = tap_finish<VT>(vc, taps[k]);
        va[k] = tf_coord(tf, sa[k]);
        aa[k] = opacity_correction<false>(tf_alpha<!POOLED>(tf, va[k]), mc.base * dts[k]);
        if (SKIP) aa[k] = mj[k] > 0.f ? aa[k] : 0.f; // a macrocell whose majorant is 0 holds no sample with opacity > 0
      }
      // ---- (3b) transparent round (wave-uniform; ~9 of 10 rounds with a sparse transfer function): no live sample of any
      //      ray of the wave has opacity > 0, so every step adds exactly 0 to alpha and colour (fma(tr, 0, x) == x) and
      //      pushes nothing - only liveness and the counters move.  The validity bits are monotone (once ty == tx == t1 it
      //      stays), so step i is live iff the ray was live at the start of the round, alpha < 0.9999 and bit i is set.
      //      (Not in the skipping kernels: they have their own, earlier fast path, and this one costs them 30 VGPRs.)
      if (!SKIP) {
        bool opaque = false;
#pragma unroll
        for (int k = 0; k < K; ++k) opaque = opaque || (aa[k] > 0.f);
        if (__ballot(opaque && live) == 0ull) {
          const bool go = live && (alpha < 0.9999f);
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const bool ml = go && ((vmask >> (4 * k + sub)) & 1u) != 0u;
            n_samples += (ml && (!SKIP || mj[k] > 0.f)) ? 1u : 0u;
            if (SKIP) n_skipped += (ml && !(mj[k] > 0.f)) ? 1u : 0u;
          }
          live = go && ((vmask >> (4 * K - 1)) & 1u) != 0u;
          continue;
        }
      }
      // (round 3) the colours of an unshaded march are only needed from here on: ~9 of 10 rounds leave through the transparent-round exit
      // above and never look them up (15 vector instructions and two 12-byte LDS reads per sample; C2 is bound by vector issue)
      if (SHADE == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const f3 rgb = tf_color(tf, va[k]);
          ca[k] = mk3(clamp01(rgb.x), clamp01(rgb.y), clamp01(rgb.z));
        }
      }
      // ---- (4) the ray's alpha recurrence over the 4K steps, in order; every lane of the quad computes all of it
      //      (a dead or zero-opacity step feeds a = 0: fma(tr, 0, alpha) == alpha exactly, so no select is needed)
      bool mlive[K], mpush[K];
      float mtr[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float al[4];   // alpha BEFORE each of the 4 steps
        bool lv[4];    // the reference's loop condition at each step, shaders_raymarching.cu:110
#define OVR_STEP(B)                                                                                                            \
        {                                                                                                                      \
          const float aj = quad_bcast<B>(aa[k]);                                                                               \
          live = live && ((vmask >> (4 * k + B)) & 1u) != 0u && (alpha < 0.9999f);                                             \
          lv[B] = live;                                                                                                        \
          al[B] = alpha;                                                                                                       \
          const float ae = live ? aj : 0.f;                                                                                    \
          const float trj = 1.f - alpha;                                                                                       \
          if (SHADE == 0) {                                                                                                    \
            const float cxj = quad_bcast<B>(ca[k].x), cyj = quad_bcast<B>(ca[k].y), czj = quad_bcast<B>(ca[k].z);              \
            color.x = fmaf(trj * cxj, ae, color.x);                                                                            \
            color.y = fmaf(trj * cyj, ae, color.y);                                                                            \
            color.z = fmaf(trj * czj, ae, color.z);                                                                            \
          }                                                                                                                    \
          alpha = fmaf(trj, ae, alpha);                                                                                        \
        }
        OVR_STEP(0) OVR_STEP(1) OVR_STEP(2) OVR_STEP(3)
#undef OVR_STEP
        mlive[k] = sub == 0 ? lv[0] : sub == 1 ? lv[1] : sub == 2 ? lv[2] : lv[3];
        mtr[k] = 1.f - sel4(al[0], al[1], al[2], al[3], subm);
        // a sample whose corrected opacity is exactly 0 adds exactly 0 to colour, gradient and alpha: nothing is shaded
        mpush[k] = mlive[k] && (aa[k] > 0.f);
      }
      // ---- (5) count; queue the samples that need shading (slot = tail + prefix of the ballot, lane order = step order)
#pragma unroll
      for (int k = 0; k < K; ++k) {
        n_samples += (mlive[k] && (!SKIP || mj[k] > 0.f)) ? 1u : 0u;
        if (SKIP) n_skipped += (mlive[k] && !(mj[k] > 0.f)) ? 1u : 0u;
        n_shaded += mpush[k] ? 1u : 0u;
        if (SHADE != 0) {
          // Quad-granular compaction: if any of a ray's 4 steps needs shading the ray takes 4 consecutive slots (the steps
          // that do not are written as null requests, a == 0, and cost the shader nothing but an idle lane).  Stream
          // positions stay multiples of 4, so in every 64-request chunk the 4 lanes of a quad shade 4 consecutive steps of
          // ONE ray: their gradient and shadow taps are 1 voxel apart and share bricks (texture-addresser coalescing).
          const bool push = mpush[k];
          const unsigned long long mp = __ballot(push);
          if (mp != 0ull) {
            const unsigned int quad_bits = (unsigned int)(mp >> qbase) & 0xfu;
            const bool qpush = quad_bits != 0u;
            const unsigned long long m = __ballot(qpush); // whole quads
            const unsigned int below = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
            if (qpush) {
              const unsigned int pos_q = q_tail + below;            // = quad_first + sub
              const unsigned int quad_first = pos_q - (unsigned int)sub;
              const unsigned int higher = quad_bits >> (sub + 1);   // later steps of this ray pushed by this instruction
              ShadeReq r;
              r.px = poss[k].x; r.py = poss[k].y; r.pz = poss[k].z;
              r.s = sa[k]; r.v = va[k]; r.tr = mtr[k];
              r.a = push ? aa[k] : 0.f;
              r.next = (push && higher != 0u) ? (int)(pos_q + 1u + (unsigned int)__builtin_ctz(higher)) : 0;
              queue[pos_q & (QCAP - 1)] = r;
              const unsigned int first_sub = (unsigned int)__builtin_ctz(quad_bits), last_sub = 31u - (unsigned int)__builtin_clz(quad_bits);
              if (push && (unsigned int)sub == first_sub && pend > 0) { // link the ray's previous request to this one
                if (!POOLED || (int)(last - q_head) >= 0) queue[last & (QCAP - 1)].next = (int)pos_q; // still in LDS
                else Q.reqs[last_gidx].next = (int)pos_q;                                              // already spilled
              }
              if (pend == 0) first = quad_first + first_sub;
              last = quad_first + last_sub;
              pend += (int)__popc(quad_bits);
            }
            q_tail += (unsigned int)__popcll(m);
            if (POOLED && (q_tail - q_head) >= 64u) spill(64u);
          }
        }
      }
    }

    // render_raymarching / alpha_blend with an always-missing background (shaders_raymarching.cu:260-321)
    if (!POOLED) {
      o_a += alpha;
      if (alpha > 0.f) {
        o_c.x += color.x / alpha; o_c.y += color.y / alpha; o_c.z += color.z / alpha;
        o_g.x += gradient.x / alpha; o_g.y += gradient.y / alpha; o_g.z += gradient.z / alpha;
      }
    }
  }

  if (POOLED) {
    if (q_tail != q_head) spill(q_tail - q_head); // the tile's last, partial chunk
    if (lane == 0 && run_ok)
      for (unsigned int i = run_size - run_left; i < run_size && run_left != 0; ++i) { // unused tail of the reservation
        Q.chunk_n[run_base + i] = 0;
        if (Q.order && ((run_base + i) & (unsigned int)(kRun - 1)) == 0u) Q.order_key[(run_base + i) / (unsigned int)kRun] = kOrderNoKey;
      }
    if (lane == 0) Q.tile_count[tile] = q_tail;
    if (active && owner) Q.pix_state[pixel_index] = make_float4(alpha, __uint_as_float(first), __int_as_float(pend), 0.f);
  }
  else if (active && owner) {
    const float rspp = 1.f / (float)spp;
    o_a *= rspp;
    o_c.x *= rspp; o_c.y *= rspp; o_c.z *= rspp;
    o_g.x *= rspp; o_g.y *= rspp; o_g.z *= rspp;
    write_pixel(P, pixel_index, o_c, o_a, o_g);
  }

  if (P.trace && lane == 0) { // diagnostic only (OVR_HIP_TRACE): per-wave residency interval and work, never read by the kernel
    unsigned long long* t = P.trace + (size_t)tile * 4;
    t[0] = t_start; t[1] = __builtin_amdgcn_s_memrealtime();
    t[2] = ((unsigned long long)n_samples << 32) | n_shaded; t[3] = n_shadow;
  }
  // LDSB (never combined with skipping): the two skip counters carry the staging diagnostics instead
  store_block_counters(P, reinterpret_cast<unsigned int*>(lds_raw), lane, wave, n_rays, n_samples, n_shaded, n_shadow,
                       (active && owner && (!POOLED || P.spp_index == 0)) ? 1u : 0u, LDSB ? n_lds_fb_taps : n_skipped,
                       LDSB ? n_lds_fb_rounds : n_shadow_skipped, n_outside_hits);
}

// ------------------------------------------------------------------------------------------------------------------
// pooled pipeline, kernel B: persistent waves shade chunks from all tiles; one returning atomic per chunk
// ------------------------------------------------------------------------------------------------------------------
template <int VT, int SHADE, int AM, bool SKIP, bool MAT, bool CLIP = false, bool CACHED = false, bool ORTHO = false>
__global__ __launch_bounds__(kBlock) void shade_pool_kernel(const RayMarchParams P)
{
  static_assert(shade_variant_exists(SHADE, AM, SKIP, MAT, CLIP, CACHED, ORTHO), "no such variant of the shade kernel (host/launch_plan.hpp)");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  TfConsts tf;
  VolConsts vc;
  MarchConsts mc;
  setup_consts(P, vc, mc);
  const size_t tb = (stage_tables<VT, AM>(P, lds_raw, vc) + 15) & ~(size_t)15; // [offset tables][TF]
  stage_tf(P, lds_raw + tb, true, tf);
  const PoolDesc& Q = P.pool;
  // runs per sub-pool; tickets enumerate them block-cyclically - kTicketBlock consecutive tickets are kTicketBlock consecutive
  // runs of ONE sub-pool (usually of one tile), the next kTicketBlock tickets belong to the next sub-pool; a ticket beyond its
  // sub-pool's runs is idle
  __shared__ unsigned int s_runs[kPoolSubs];
  __shared__ unsigned int s_tot[2];
  if (threadIdx.x < (unsigned int)kPoolSubs) s_runs[threadIdx.x] = min(Q.ctrl[32u * (threadIdx.x + 1u)], Q.sub_capacity) / (unsigned int)kRun;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int mx = 0, sum = 0;
    for (int i = 0; i < kPoolSubs; ++i) { mx = max(mx, s_runs[i]); sum += s_runs[i]; }
    s_tot[0] = mx; s_tot[1] = sum;
  }
  __syncthreads();
  const bool overflow = Q.ctrl[1] != 0u; // a sub-pool ran out: the frame is re-rendered, nothing to shade
  const unsigned int total_runs = overflow ? 0u : s_tot[1];
  const unsigned int n_runs = overflow ? 0u : ((s_tot[0] + kTicketBlock - 1) / kTicketBlock) * kTicketBlock * (unsigned int)kPoolSubs; // tickets
  unsigned int n_shadow = 0, n_shadow_skipped = 0;
  __shared__ unsigned int s_run;
  // Guided self-scheduling: a workgroup takes a BATCH of consecutive runs per ticket - (runs left) / (2 x workgroups), at most
  // kTicketRuns, at least 1 - because the ticket is a same-address returning atomic and those serialise in L2 (~30 clocks each:
  // with one run per ticket the dense-transfer-function frame spent its whole shade time on 116 k tickets).  Large batches while
  // there is plenty of work, single runs at the end for balance.  Inside a batch the 4 waves walk their chunks independently
  // (run r, chunk `wave`): consecutive depth steps of ONE tile, whose gradient and shadow taps fall into the same bricks.
  // The cap follows the frame: 1 run per ticket up to 32 runs per workgroup (sparse transfer functions: 36 k runs per C3 frame -
  // there batches only cost balance, measured +3 ... 13 %), up to kTicketRuns beyond (dense: 174 k runs, shade 2.11 -> 1.13 ms)
  // Without the shadow march (SHADE == 1) a run is three gradient taps per request - so cheap that even 36 k single-run tickets ARE the
  // kernel's time (0.45 ms on C3: ~16 ns per same-address atomic); there the cap is always kTicketRuns (shade 0.45 -> 0.20 ms, profiles/r02_notes.md §11)
  // (with the shadow march the batches cost more in balance and locality than the tickets do - also in the skipping kernel: 0.668 -> 0.729 ms)
  const unsigned int ticket_cap = SHADE == 1 ? (unsigned int)kTicketRuns : min((unsigned int)kTicketRuns, max(1u, total_runs / (32u * gridDim.x)));
  auto shade_chunk = [&](unsigned int c) {
    const unsigned int n = Q.chunk_n[c];
    if ((unsigned int)lane < n) {
      ShadeReq r = Q.reqs[(size_t)c * 64 + lane];
      if (r.a > 0.f) { // a == 0: null request (a step of the quad that needs no shading)
        shade_request<VT, SHADE, AM, SKIP, MAT, CLIP, CACHED, ORTHO>(P, vc, tf, mc, r, n_shadow, n_shadow_skipped);
        Q.reqs[(size_t)c * 64 + lane] = r;
      }
    }
  };
  if (Q.order) {
    // (the next generation's march counts into a zeroed histogram; the order kernel's fill counters likewise)
    for (unsigned int i = blockIdx.x * kBlock + threadIdx.x; i < 2u * (unsigned int)kOrderMaxKeys; i += gridDim.x * kBlock) {
      const unsigned int e = i < (unsigned int)kOrderMaxKeys ? i : i - (unsigned int)kOrderMaxKeys;
      if (e < (unsigned int)(Q.order_grid * Q.order_grid)) Q.order_ws[i] = 0u;
    }
    // Runs sorted by light beam (PoolDesc::order, shade_order_kernel): 8 lists with a ticket counter each; the workgroups of an XCD start on
    // "their" list, so the bricks a beam's shadow rays sweep are fetched into ONE L2 and hit there by the beam's later runs; a workgroup whose
    // list is done helps with the others (the cursors only grow: every workgroup passes every list once and leaves)
    const unsigned int* ls = Q.order_ws + kOrderListStart;
    unsigned int* tick = Q.order_ws + kOrderTickets;
    unsigned int xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
    const unsigned int total = overflow ? 0u : ls[kOrderLists];
    const unsigned int cap = SHADE == 1 ? (unsigned int)kTicketRuns : min((unsigned int)kTicketRuns, max(1u, total / (32u * gridDim.x)));
    const unsigned int wgs = max(1u, gridDim.x / (unsigned int)kOrderLists);
    for (unsigned int li = 0; li < (unsigned int)kOrderLists; ++li) {
      const unsigned int l = (xcc + li) & (unsigned int)(kOrderLists - 1);
      const unsigned int beg = ls[l], n_l = overflow ? 0u : ls[l + 1] - beg;
      unsigned int seen = 0;
      for (;;) {
        const unsigned int left = n_l > seen ? n_l - seen : 0u;
        const unsigned int batch = min(cap, max(1u, left / (2u * wgs)));
        __syncthreads();
        if (threadIdx.x == 0) s_run = atomicAdd(&tick[32u * l], batch);
        __syncthreads();
        const unsigned int run0 = s_run;
        if (run0 >= n_l) break;
        seen = run0 + batch;
        const unsigned int run1 = min(run0 + batch, n_l);
        for (unsigned int ticket = run0; ticket < run1; ++ticket) {
          if (ticket != run0) __syncthreads(); // the 4 waves stay on ONE run
          const unsigned int c0 = Q.order[beg + ticket] * (unsigned int)kRun;
          for (unsigned int i = (unsigned int)wave; i < (unsigned int)kRun; i += kWaves) shade_chunk(c0 + i);
        }
      }
    }
  }
  else {
  unsigned int seen = 0; // a lower bound of the global cursor: the end of this workgroup's last batch
  for (;;) {
    const unsigned int left = n_runs > seen ? n_runs - seen : 0u;
    const unsigned int batch = min(ticket_cap, max(1u, left / (2u * gridDim.x)));
    __syncthreads();
    if (threadIdx.x == 0) s_run = atomicAdd(&Q.ctrl[0], batch);
    __syncthreads();
    const unsigned int run0 = s_run;
    if (run0 >= n_runs) break; // every workgroup reaches this: the cursor only grows
    seen = run0 + batch;
    const unsigned int run1 = min(run0 + batch, n_runs);
    for (unsigned int ticket = run0; ticket < run1; ++ticket) {
      if (ticket != run0) __syncthreads(); // the 4 waves stay on ONE run: its chunks share their bricks in L1
      const unsigned int grp = ticket / kTicketBlock, sub = grp & (unsigned int)(kPoolSubs - 1);
      const unsigned int run = (grp / (unsigned int)kPoolSubs) * kTicketBlock + ticket % kTicketBlock;
      if (run >= s_runs[sub]) continue; // idle ticket (workgroup-uniform)
      for (unsigned int i = (unsigned int)wave; i < (unsigned int)kRun; i += kWaves) shade_chunk(sub * Q.sub_capacity + run * kRun + i);
    }
  }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_shadow += __shfl_down(n_shadow, off);
    n_shadow_skipped += __shfl_down(n_shadow_skipped, off);
  }
  __syncthreads();
  unsigned int* red = reinterpret_cast<unsigned int*>(lds_raw);
  if (lane == 0) { red[wave] = n_shadow; red[kWaves + wave] = n_shadow_skipped; }
  __syncthreads();
  if (threadIdx.x == 0 && Q.shade_counters) {
    Q.shade_counters[2 * blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    Q.shade_counters[2 * blockIdx.x + 1] = red[4] + red[5] + red[6] + red[7];
  }
}


// ------------------------------------------------------------------------------------------------------------------
// a launch plan's two kernels.  SHADE comes from a switch, AM from dispatch_addressing, the plan's flags become template arguments through ONE constant, a set of
// bits: every combination for which march_variant_exists / shade_variant_exists (host/launch_plan.hpp) holds is instantiated, and nothing else
// ------------------------------------------------------------------------------------------------------------------
typedef void (*FrameKernel)(const RayMarchParams);
struct FrameKernels { FrameKernel march = nullptr, shade = nullptr; }; // shade: pooled plans only; march == nullptr: no such variant of this type
enum VariantBits : unsigned { kBitPooled = 1, kBitSkip = 2, kBitLdsStaged = 4, kBitDeep = 8, kBitMaterial = 16, kBitClipped = 32, kBitCached = 64,
                     kBitOrtho = 128, kVariantBitsEnd = 256 };
constexpr unsigned kShadeBits = kBitSkip | kBitMaterial | kBitClipped | kBitCached | kBitOrtho; // the flags shade_pool_kernel has

template <int VT, int SHADE, int AM, unsigned BITS>
constexpr FrameKernel march_variant()
{
  constexpr bool pooled = BITS & kBitPooled, skip = BITS & kBitSkip, lds_staged = BITS & kBitLdsStaged, deep = BITS & kBitDeep, material = BITS & kBitMaterial,
                 clipped = BITS & kBitClipped, cached = BITS & kBitCached, ortho = BITS & kBitOrtho;
  if constexpr (march_variant_exists(SHADE, AM, pooled, skip, lds_staged, deep, material, clipped, VT == VOX_F32, cached, ortho))
    return raymarch_kernel<VT, SHADE, AM, pooled, skip, lds_staged, deep, material, clipped, cached, ortho>;
  else return nullptr;
}
template <int VT, int SHADE, int AM, unsigned BITS>
constexpr FrameKernel shade_variant()
{
  constexpr bool skip = BITS & kBitSkip, material = BITS & kBitMaterial, clipped = BITS & kBitClipped, cached = BITS & kBitCached, ortho = BITS & kBitOrtho;
  if constexpr ((BITS & ~kShadeBits) == 0 && shade_variant_exists(SHADE, AM, skip, material, clipped, cached, ortho))
    return shade_pool_kernel<VT, SHADE, AM, skip, material, clipped, cached, ortho>;
  else return nullptr;
}
// a run-time addressing mode as a compile-time one: f(std::integral_constant<int, AM>{}) for the modes the voxel type's kernels exist at - 0 to 3, and 4 exactly
// where row_load_layout (host/launch_plan.hpp) holds for the type.  R() - no such variant - for any other mode, and with GENERAL_ONLY for a replica's type: the
// kernels that exist for the general layouts alone (the layout that is always resident) are looked up through it, as dispatch_voxel_type<true> names their types
template <typename R, int VT, bool GENERAL_ONLY = false, typename F>
inline R dispatch_addressing(int am, F&& f)
{
  if constexpr (!GENERAL_ONLY || kVoxelTypes[VT].layout == LAYOUT_GENERAL) {
    switch (am) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4:
      if constexpr (row_load_layout((int)sizeof(typename Vox<VT>::T), Vox<VT>::kQuad)) { // (mode 4 is RowLoads' own)
        static_assert(RowLoads<VT, 4>::on, "row_load_layout (host/launch_plan.hpp) names the layouts RowLoads is on for");
        return f(std::integral_constant<int, 4>{});
      }
    }
  }
  return R();
}
// entry i of the table { G::at<0>(), G::at<1>(), ... }: a lookup's variants by ONE constant, each entry an `if constexpr (<the predicate of host/launch_plan.hpp>)
// <the kernel> else nullptr` - the predicate decides which kernels are instantiated
template <typename G, unsigned... I>
inline auto variant_at(unsigned i, std::integer_sequence<unsigned, I...>) -> decltype(G::template at<0>())
{
  static constexpr decltype(G::template at<0>()) table[] = { G::template at<I>()... };
  return table[i];
}

template <int VT, int SHADE, int AM, unsigned... BITS>
inline FrameKernels variants_of(unsigned march_bits, unsigned shade_bits, std::integer_sequence<unsigned, BITS...>)
{
  static constexpr FrameKernel march[] = { march_variant<VT, SHADE, AM, BITS>()... }, shade[] = { shade_variant<VT, SHADE, AM, BITS>()... };
  return { march[march_bits], shade[shade_bits] };
}
template <int VT, int SHADE>
inline FrameKernels variants_of(int am, unsigned march_bits, unsigned shade_bits)
{
  return dispatch_addressing<FrameKernels, VT>(am, [&](auto m) {
    return variants_of<VT, SHADE, decltype(m)::value>(march_bits, shade_bits, std::make_integer_sequence<unsigned, kVariantBitsEnd>());
  });
}

// ------------------------------------------------------------------------------------------------------------------
// the shadow cache's build kernel (ShadowBuildArgs in ovr_hip_kernels.h): one lane per node, a wave = a 4 x 4 x 4 tile of nodes - neighbours in all three
// directions, so the lanes' shadow rays sweep the same bricks -, or one lane per caller-supplied position.  Transfer function (alphas only) and axis tables
// are staged as shade_pool_kernel stages them.  CLIP = true only: the bounds (0, 1) give the literal test's bits.  Instantiated for
// the general layouts - the layout that is always resident and that ovr_hip_update_volume rewrites first.
// ------------------------------------------------------------------------------------------------------------------
template <int VT, int AM>
__global__ __launch_bounds__(kBlock) void shadow_cache_kernel(const RayMarchParams P, const ShadowBuildArgs A)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  TfConsts tf;
  VolConsts vc;
  MarchConsts mc;
  setup_consts(P, vc, mc);
  const size_t tb = (stage_tables<VT, AM>(P, lds_raw, vc) + 15) & ~(size_t)15; // [offset tables][alphas]
  stage_tf(P, lds_raw + tb, false, tf);
  bool valid;
  long long index;
  f3 org = mk3(0.f, 0.f, 0.f);
  if (A.pos) {
    index = (long long)blockIdx.x * kBlock + threadIdx.x;
    valid = index < A.n;
    if (valid) org = mk3(A.pos[3 * index], A.pos[3 * index + 1], A.pos[3 * index + 2]);
  }
  else {
    const long long tx = (A.nx + 3) / 4, ty = (A.ny + 3) / 4;
    const long long tile = (long long)blockIdx.x * kWaves + wave;
    const int ix = (int)(tile % tx) * 4 + (lane & 3), iy = (int)((tile / tx) % ty) * 4 + ((lane >> 2) & 3);
    const long long izl = (tile / (tx * ty)) * 4 + (lane >> 4);
    valid = ix < A.nx && iy < A.ny && izl < (long long)A.nz;
    const int iz = (int)izl;
    index = (long long)ix + (long long)A.nx * ((long long)iy + (long long)A.ny * (long long)iz);
    const float ux = (float)ix / (float)(A.nx - 1), uy = (float)iy / (float)(A.ny - 1), uz = (float)iz / (float)(A.nz - 1);
    org = mk3(fmaf(ux, A.sc[0], A.origin[0]), fmaf(uy, A.sc[1], A.origin[1]), fmaf(uz, A.sc[2], A.origin[2]));
  }
  unsigned int n_shadow = 0, n_shadow_skipped = 0;
  if (valid) {
    if (A.out) A.out[index] = march_shadow<VT, AM, kShadowTaps, false, true>(P, vc, tf, mc, org, n_shadow, n_shadow_skipped); // (null: the positions alone)
    if (A.pos_out) { A.pos_out[3 * index] = org.x; A.pos_out[3 * index + 1] = org.y; A.pos_out[3 * index + 2] = org.z; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n_shadow += __shfl_down(n_shadow, off);
  if (lane == 0 && A.iterations && n_shadow) atomicAdd(A.iterations, (unsigned long long)n_shadow);
}
typedef void (*ShadowCacheKernel)(const RayMarchParams, const ShadowBuildArgs);
// the build kernel of a voxel type at an addressing mode; nullptr for a replica's type (or mode 4 on a layout without row loads)
template <int VT>
ShadowCacheKernel shadow_cache_kernel_of(int am)
{
  return dispatch_addressing<ShadowCacheKernel, VT, true>(am, [](auto m) -> ShadowCacheKernel { return shadow_cache_kernel<VT, decltype(m)::value>; });
}

// ------------------------------------------------------------------------------------------------------------------
// projections (include/ovr_hip.h ovr_hip_set_projection; open-volume-renderer_amd/projection.py is the normative arithmetic): per ray the
// maximum, the minimum or the mean of the samples the unshaded march would classify - the march without its sequential part: no opacity recurrence, no early
// termination, no pow, no transfer-function lookup per sample, ONE classification per ray (read from global memory: 64 rays x 6 loads per workgroup against
// 20 KB of staged tables; LDS holds the axis tables alone).  The work decomposition is the march's: four lanes per ray = four consecutive steps (the quad
// coalescing of the texture addresser, raymarch_kernel's header), every lane runs the (tx, ty) recurrence, a round = kProjectK instructions x 4 steps with all
// its voxel loads in flight before the first is consumed.  Lane `sub` owns the steps i with i & 3 == sub: its running extremum (first of equal samples: the
// strict comparison) or its sum IS the definition's accumulator A[i & 3]; the quad is combined once, behind the loop.
// SKIP (maximum / minimum): a step's fetch is dropped when the value range of its tap's macrocell (RayMarchParams::mc_ranges, tap_cell) proves that the sample
// cannot replace the extremum.  Two things make the test exact rather than approximate:
//  * the filter rounds: a sample can leave the range of the voxels it reads.  range_slack bounds by how much (derivation: DESIGN.md section 16) - three levels of
//    fmaf(f, b - a, a), each off by at most u (width + magnitude) with u = 2^-24, the 8-bit types' normalisation behind the filter and the rounding of the bound
//    itself: below 7 u (W + M), taken as 2^-21 (W + M) so that the product is exact, plus FLT_MIN for gradual underflow;
//  * ties decide tm*: the bound is the quad's extremum over the rounds BEFORE this one (shared with DPP quad broadcasts between rounds, as the march shares
//    opacities) - every step it comes from is earlier than every step of this round, so an equal sample never replaces it and `<=` is exact.  What another lane
//    finds in the SAME round is not used as a bound (it is not earlier; it would need the strict comparison and a second exchange per round).
// The frame, the layer and samples + skipped_samples are bit for bit the non-skipping kernel's.  Measured: profiles/r14_projection.md.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float range_slack(float lo, float hi) { return fmaf(0x1p-21f, (hi - lo) + fmaxf(fabsf(lo), fabsf(hi)), FLT_MIN); }

struct ProjectResult {
  float v, tm;                          // the projected value and the distance of the sample that set it (0 for the mean); quad-uniform
  unsigned int steps;                   // n, quad-uniform
  unsigned int fetched, skipped;        // THIS LANE's steps whose voxels were fetched / whose fetch was skipped
};

// the ray org + t dir (world space, as the march forms it) over [t0, t1]; live: the ray is marched (quad-uniform)
template <int VT, int AM, int MODE, bool SKIP>
__device__ __forceinline__ ProjectResult project_ray(const RayMarchParams& P, const VolConsts& vc, const MarchConsts& mc, f3 org, f3 dir, float t0, float t1, bool live,
                                                     const SubMask& subm)
{
  static_assert(project_variant_exists(MODE, AM, SKIP, false), "no such variant of the projection (host/launch_plan.hpp)");
  constexpr int K = kProjectK;
  constexpr bool MAXI = MODE == kProjectMaximum, MEAN = MODE == kProjectMean;
  const int sub = subm.sub;
  float m = MAXI ? -__builtin_inff() : __builtin_inff(), tmb = 0.f; // this lane's extremum over its own steps
  float bound = m;                                                   // SKIP: the quad's extremum over the earlier rounds
  float acc = 0.f;                                                   // mean: A[sub]
  unsigned int own = 0, fetched = 0, skipped = 0;
  float tx = t0, ty = fminf(t1, t0 + mc.step);
  while (__ballot(live) != 0ull) {
    unsigned int vmask = 0;
    float tms[K];
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
      tms[k] = 0.5f * (sel4(txq[0], txq[1], txq[2], txq[3], subm) + sel4(tyq[0], tyq[1], tyq[2], tyq[3], subm));
    }
    Tap taps[K];
    bool fetch[K];
    bool any = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const f3 pos = mk3(fmaf(tms[k], dir.x, org.x), fmaf(tms[k], dir.y, org.y), fmaf(tms[k], dir.z, org.z));
      if (SKIP) taps[k] = Tap{}; // (a tap that is not fetched is finished all the same, and dropped)
      tap_coords(vc, to_object(mc, pos), taps[k]);
      const bool mine = live && ((vmask >> (4 * k + sub)) & 1u) != 0u;
      fetch[k] = mine;
      if (SKIP) {
        const float2 r = reinterpret_cast<const float2*>(P.mc_ranges)[tap_cell(vc, taps[k])];
        const float sl = range_slack(r.x, r.y);
        const bool cannot = MAXI ? (r.y + sl <= bound) : (r.x - sl >= bound); // (a NaN range proves nothing)
        fetch[k] = mine && !cannot;
        skipped += (mine && cannot) ? 1u : 0u;
      }
      own += mine ? 1u : 0u;
      fetched += fetch[k] ? 1u : 0u;
      any = any || fetch[k];
    }
    live = live && ((vmask >> (4 * K - 1)) & 1u) != 0u; // validity is monotone: the round's last step decides whether another round exists
    if (SKIP) {
      if (__ballot(any) == 0ull) continue; // nothing to fetch for any lane of the wave: the extrema stand
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (fetch[k]) tap_loads<VT, AM>(vc, taps[k]);
    }
    else {
      // branch-free, like the march: dead lanes load (their coordinates are clamped, the loads are in bounds) and drop the value
#pragma unroll
      for (int k = 0; k < K; ++k) tap_loads<VT, AM>(vc, taps[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float s = tap_finish<VT>(vc, taps[k]);
      if (MEAN) acc = fetch[k] ? acc + s : acc;
      else {
        const bool take = fetch[k] && (MAXI ? s > m : s < m); // strict: of equal samples the first stays; a NaN is never selected
        m = take ? s : m;
        tmb = take ? tms[k] : tmb;
      }
    }
    if (SKIP) {
      const float b0 = quad_bcast<0>(m), b1 = quad_bcast<1>(m), b2 = quad_bcast<2>(m), b3 = quad_bcast<3>(m);
      bound = MAXI ? fmaxf(fmaxf(b0, b1), fmaxf(b2, b3)) : fminf(fminf(b0, b1), fminf(b2, b3));
    }
  }
  ProjectResult res;
  {
    const float o = __uint_as_float(own);
    res.steps = __float_as_uint(quad_bcast<0>(o)) + __float_as_uint(quad_bcast<1>(o)) + __float_as_uint(quad_bcast<2>(o)) + __float_as_uint(quad_bcast<3>(o));
  }
  res.fetched = fetched;
  res.skipped = skipped;
  if (MEAN) {
    const float a0 = quad_bcast<0>(acc), a1 = quad_bcast<1>(acc), a2 = quad_bcast<2>(acc), a3 = quad_bcast<3>(acc);
    res.v = ((a0 + a1) + (a2 + a3)) / (float)res.steps;
    res.tm = 0.f;
  }
  else {
    // the larger (smaller) value; of equal values the smaller tm - the earlier step
    float bv = quad_bcast<0>(m), bt = quad_bcast<0>(tmb);
#define OVR_COMBINE(B)                                                                                                 \
    {                                                                                                                  \
      const float cv = quad_bcast<B>(m), ct = quad_bcast<B>(tmb);                                                      \
      const bool take = (MAXI ? cv > bv : cv < bv) || (cv == bv && ct < bt);                                           \
      bv = take ? cv : bv;                                                                                             \
      bt = take ? ct : bt;                                                                                             \
    }
    OVR_COMBINE(1) OVR_COMBINE(2) OVR_COMBINE(3)
#undef OVR_COMBINE
    res.v = bv;
    res.tm = bt;
  }
  return res;
}

// the classification of a projected value, once per ray, from the tables in global memory: the march's tf_coord and nodal lerps (the pair (i0, min(i0 + 1,
// n - 1)) is the padded tables' (i0, i0 + 1): i0 = n - 1 only for a fraction of 0)
__device__ __forceinline__ float4 project_classify(const RayMarchParams& P, float v)
{
  const float c = clamp01((fminf(fmaxf(v, P.tf_lower), P.tf_upper) - P.tf_lower) * P.tf_scale);
  const int nc1 = P.n_color - 1, na1 = P.n_alpha - 1;
  const float xc = c * (float)nc1, xa = c * (float)na1;
  const int ic = (int)xc, ia = (int)xa;
  const float fc = __builtin_amdgcn_fractf(xc), fa = __builtin_amdgcn_fractf(xa);
  const float4* col = reinterpret_cast<const float4*>(P.tf_color);
  const float4 a = col[ic], b = col[min(ic + 1, nc1)];
  return make_float4(clamp01(lerpf(a.x, b.x, fc)), clamp01(lerpf(a.y, b.y, fc)), clamp01(lerpf(a.z, b.z, fc)), lerpf(P.tf_alpha[ia], P.tf_alpha[min(ia + 1, na1)], fa));
}

// a projection frame: the march's pixels, block schedule, sparse list, samples per pixel, jitter and write_pixel around project_ray; the buffer mapframe hands
// out as `grad` carries the projection layer (v, tm*, 1).  No request queue, no alpha, no occupancy attribute (none is measured to pay)
// ORTHO: the orthographic camera's rays (pixel_ray) - on the clipped variants alone
template <int VT, int AM, int MODE, bool SKIP, bool CLIP, bool ORTHO = false>
__global__ __launch_bounds__(kBlock) void project_kernel(const RayMarchParams P)
{
  static_assert(project_variant_exists(MODE, AM, SKIP, CLIP, ORTHO) && (AM != 4 || RowLoads<VT, 4>::on), "no such variant of the projection (host/launch_plan.hpp)");
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
  if (__syncthreads_or(active ? 1 : 0) != 0) {
    stage_tables<VT, AM>(P, lds_raw, vc);
    __syncthreads();
  }
  else {
    vc.tab_x = vc.tab_y = vc.tab_z = nullptr;
    vc.tab_z64 = nullptr;
  }
  unsigned int n_rays = 0, n_samples = 0, n_skipped = 0, n_outside_hits = 0;
  const float rsx = 1.f / (float)P.width, rsy = 1.f / (float)P.height;
  const float scx = ((float)ix + .5f) * rsx, scy = ((float)iy + .5f) * rsy;
  const unsigned int pixel_index = (unsigned int)ix + (unsigned int)iy * (unsigned int)P.width;
  unsigned int v0 = (unsigned int)P.frame_index, v1 = pixel_index; // RandomTEA(frame_index, pixel_index)
  float o_a = 0.f;
  f3 o_c = mk3(0, 0, 0), o_g = mk3(0, 0, 0);
  for (int k_spp = 0; k_spp < P.spp; ++k_spp) { // uniform trip count
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
    const ProjectResult pr = project_ray<VT, AM, MODE, SKIP>(P, vc, mc, org, dir, t0, t1, live, subm);
    n_samples += pr.fetched;
    n_skipped += pr.skipped;
    if (live && owner && pr.steps > 0u) {
      const float4 c = project_classify(P, pr.v);
      o_c.x += c.x; o_c.y += c.y; o_c.z += c.z;
      o_a += c.w;
      o_g.x += pr.v; o_g.y += pr.tm; o_g.z += 1.f;
    }
  }
  if (active && owner) {
    const float rspp = 1.f / (float)P.spp;
    o_a *= rspp;
    o_c.x *= rspp; o_c.y *= rspp; o_c.z *= rspp;
    o_g.x *= rspp; o_g.y *= rspp; o_g.z *= rspp;
    write_pixel(P, pixel_index, o_c, o_a, o_g);
  }
  store_block_counters(P, reinterpret_cast<unsigned int*>(lds_raw), lane, wave, n_rays, n_samples, 0u, 0u, (active && owner) ? 1u : 0u, n_skipped, 0u, n_outside_hits);
}

// the known-answer entry's kernel: ray i = the quad of lanes 4 i ... 4 i + 3, through project_ray as the frame's kernel calls it.  The clipped box test alone: the
// bounds (0, 1) without a clip box give the unclipped test's bits
template <int VT, int AM, int MODE, bool SKIP>
__global__ __launch_bounds__(kBlock) void project_floats_kernel(const RayMarchParams P, const float* org, const float* dir, float* out, long long n)
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
  const ProjectResult pr = project_ray<VT, AM, MODE, SKIP>(P, vc, mc, o, d, t0, t1, live, subm);
  const float f = __uint_as_float(pr.fetched);
  const unsigned int fetched = __float_as_uint(quad_bcast<0>(f)) + __float_as_uint(quad_bcast<1>(f)) + __float_as_uint(quad_bcast<2>(f)) + __float_as_uint(quad_bcast<3>(f));
  if (valid && sub == 0) {
    const bool hit = live && pr.steps > 0u;
    out[4 * i] = hit ? pr.v : 0.f; out[4 * i + 1] = hit ? pr.tm : 0.f;
    out[4 * i + 2] = hit ? (float)pr.steps : 0.f; out[4 * i + 3] = hit ? (float)fetched : 0.f;
  }
}

typedef void (*ProjectFloatsKernel)(const RayMarchParams, const float*, const float*, float*, long long);
struct ProjectKernels { FrameKernel frame = nullptr; ProjectFloatsKernel floats = nullptr; }; // nullptr: no such variant of this type
// the flags of a projection's or an isosurface's variant as one constant: these bits, above them the mode (from kProjectMaximum) or the shading mode
enum WalkBits : unsigned { kWalkSkip = 1, kWalkClipped = 2, kWalkOrtho = 4, kWalkBitsEnd = 8 };
inline unsigned walk_bits(bool skip, bool clipped, bool ortho) { return (skip ? kWalkSkip : 0u) | (clipped ? kWalkClipped : 0u) | (ortho ? kWalkOrtho : 0u); }
template <int VT, int AM> struct ProjectVariants {
  template <unsigned I> static constexpr ProjectKernels at()
  {
    constexpr int mode = kProjectMaximum + (int)(I / kWalkBitsEnd);
    constexpr bool skip = I & kWalkSkip, clipped = I & kWalkClipped, ortho = I & kWalkOrtho;
    if constexpr (project_variant_exists(mode, AM, skip, clipped, ortho)) return { project_kernel<VT, AM, mode, skip, clipped, ortho>, project_floats_kernel<VT, AM, mode, skip> };
    else return {};
  }
};
// a projection plan's kernels of a voxel type; nullptr for a replica's type (or mode 4 on a layout without row loads), like shadow_cache_kernel_of
template <int VT>
ProjectKernels project_kernels_of(const LaunchPlan& pl)
{
  constexpr unsigned n = (kProjectMean - kProjectMaximum + 1) * kWalkBitsEnd;
  const unsigned i = (unsigned)(pl.project.mode - kProjectMaximum) * kWalkBitsEnd + walk_bits(pl.project.skip, pl.project.clipped, pl.orthographic);
  if (pl.error || i >= n) return ProjectKernels(); // (a plan without a projection: mode 0)
  return dispatch_addressing<ProjectKernels, VT, true>(pl.am, [&](auto m) { return variant_at<ProjectVariants<VT, decltype(m)::value>>(i, std::make_integer_sequence<unsigned, n>()); });
}

// ------------------------------------------------------------------------------------------------------------------
// isosurfaces (include/ovr_hip.h ovr_hip_set_isosurfaces; open-volume-renderer_amd/isosurface.py is the normative arithmetic): opaque,
// shaded, hard-shadowed level sets for up to four isovalues - the projection's walk with another reduction and an early exit.  side(s) = #{k : iso_k <= s}; the
// hit is the first step whose side differs from its predecessor's.  Lane `sub` owns the steps i with i & 3 == sub, as in project_ray; the predecessor's side comes
// from the lane to the left (one quad permute), lane 0 takes lane 3's of the instruction before, carried across rounds.  The quad's first crossing is the smallest
// crossing step among its lanes; `live` drops for the whole quad behind the round that holds it.  Every loop is bounded by the ray's step count.
// SKIP: a step's fetch is dropped when no isovalue lies in [lo - S, hi + S] of its tap's macrocell (range_slack); its side is then #{k : iso_k < lo - S}, the side
// of every sample the cell can produce.  The two samples of the hit's pair are tapped again behind the walk (lanes 0 and 1, one instruction) - the walk's bits, and
// there whether the walk fetched them or not.
// Refinement: a round is ONE tap per lane (p_1 ... p_4) and four quad broadcasts; s* and the three gradient taps are one instruction too (lanes 0 ... 3).
// Dead and finished lanes keep tapping: every position goes through tap_coords, which clamps it, so every load is in bounds.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int quad_bcast_i(int x, int b) // value of lane b (quad-uniform, 0 ... 3) of this lane's quad
{
  const int b0 = __builtin_amdgcn_update_dpp(0, x, 0x00, 0xf, 0xf, true), b1 = __builtin_amdgcn_update_dpp(0, x, 0x55, 0xf, 0xf, true);
  const int b2 = __builtin_amdgcn_update_dpp(0, x, 0xaa, 0xf, 0xf, true), b3 = __builtin_amdgcn_update_dpp(0, x, 0xff, 0xf, 0xf, true);
  return b == 0 ? b0 : b == 1 ? b1 : b == 2 ? b2 : b3;
}
__device__ __forceinline__ float quad_pick(float x, int b) { return __int_as_float(quad_bcast_i(__float_as_int(x), b)); }
// the value of the lane to the left in the quad (quad_perm [0, 0, 1, 2]): lane 0 keeps its own
__device__ __forceinline__ int quad_left_i(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x90, 0xf, 0xf, true); }

__device__ __forceinline__ int iso_side(const RayMarchParams& P, float s) // a NaN compares false: side 0
{
  int n = 0;
#pragma unroll
  for (int k = 0; k < kMaxIsovalues; ++k) n += (k < P.iso_n && P.iso_values[k] <= s) ? 1 : 0;
  return n;
}

struct IsoWalk {
  bool hit;                       // quad-uniform, like ta ... steps
  float ta, tb;                   // tm_{i-1}, tm_i of the hit's pair
  int side_a, side_b;             // their sides
  unsigned int steps;             // steps walked: i + 1 on a hit, n on a miss
  unsigned int fetched, skipped;  // THIS LANE's walked steps whose voxels were fetched / whose fetch was dropped
};

// what a resumed walk takes over from the walk before it (the translucent isosurfaces).  In: the side and tm of the step before the walk's
// first one - the hit step of the walk before (side -1: there is none).  Out, on a hit: the hit step's ty, where the next walk's recurrence goes on
// (tx_{i+1} = ty_i, CONTINUED, never recomputed from tm).  A resumed walk deals its steps to the lanes from its own start: the definition is per step
struct IsoCarry { int side; float tm, ty; };

// the first crossing along org + t dir: steps by the projection's recurrence from tx = tx0 to t1; live: the ray is walked (quad-uniform)
// RESUME: the walk may continue another one (carry), and hands back what the next one needs
template <int VT, int AM, bool SKIP, bool RESUME = false>
__device__ __forceinline__ IsoWalk iso_walk(const RayMarchParams& P, const VolConsts& vc, const MarchConsts& mc, f3 org, f3 dir, float tx0, float t1, bool live,
                                            const SubMask& subm, IsoCarry* carry = nullptr)
{
  constexpr int K = kProjectK;
  const int sub = subm.sub;
  IsoWalk w;
  w.hit = false; w.ta = w.tb = 0.f; w.side_a = w.side_b = 0; w.steps = 0u; w.fetched = w.skipped = 0u;
  unsigned int own = 0;
  int carry_side = -1; // the side of the step before the round's first; -1: there is none (step 0 has no predecessor)
  float carry_tm = 0.f;
  if constexpr (RESUME) { carry_side = carry->side; carry_tm = carry->tm; }
  float tx = tx0, ty = fminf(t1, tx0 + mc.step);
  while (__ballot(live) != 0ull) {
    unsigned int vmask = 0;
    float tms[K];
    [[maybe_unused]] float tys[K]; // RESUME: this lane's steps' ty
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
      tms[k] = 0.5f * (sel4(txq[0], txq[1], txq[2], txq[3], subm) + sel4(tyq[0], tyq[1], tyq[2], tyq[3], subm));
      if constexpr (RESUME) tys[k] = sel4(tyq[0], tyq[1], tyq[2], tyq[3], subm);
    }
    Tap taps[K];
    bool mine[K], fetch[K];
    int sd[K];
    bool any = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const f3 pos = mk3(fmaf(tms[k], dir.x, org.x), fmaf(tms[k], dir.y, org.y), fmaf(tms[k], dir.z, org.z));
      if (SKIP) taps[k] = Tap{}; // (a tap that is not fetched is finished all the same, and dropped)
      tap_coords(vc, to_object(mc, pos), taps[k]);
      mine[k] = live && ((vmask >> (4 * k + sub)) & 1u) != 0u;
      fetch[k] = mine[k];
      sd[k] = 0;
      if (SKIP) {
        const float2 r = reinterpret_cast<const float2*>(P.mc_ranges)[tap_cell(vc, taps[k])];
        const float sl = range_slack(r.x, r.y);
        const float a = r.x - sl, b = r.y + sl;
        bool drop = true; // (a NaN bound proves nothing: both comparisons fail)
        int below = 0;
#pragma unroll
        for (int j = 0; j < kMaxIsovalues; ++j) {
          const bool lt = j < P.iso_n && P.iso_values[j] < a, gt = P.iso_values[j] > b;
          drop = drop && (j >= P.iso_n || lt || gt);
          below += lt ? 1 : 0;
        }
        fetch[k] = mine[k] && !drop;
        sd[k] = below;
      }
      any = any || fetch[k];
    }
    const bool more = ((vmask >> (4 * K - 1)) & 1u) != 0u; // validity is monotone: the round's last step decides whether another round exists
    if (SKIP) {
      if (__ballot(any) != 0ull) {
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (fetch[k]) tap_loads<VT, AM>(vc, taps[k]);
      }
    }
    else {
      // branch-free, like the projection: dead lanes load (their coordinates are clamped, the loads are in bounds) and drop the value
#pragma unroll
      for (int k = 0; k < K; ++k) tap_loads<VT, AM>(vc, taps[k]);
    }
    int lsd[K];
    int cand = 4 * K; // this lane's first crossing of the round, as a step of the round; 4 K: none
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int ss = iso_side(P, tap_finish<VT>(vc, taps[k]));
      if (!SKIP || fetch[k]) sd[k] = ss;
    }
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {
      const int left = quad_left_i(sd[k]);
      const int before = k == 0 ? carry_side : __builtin_amdgcn_update_dpp(0, sd[k > 0 ? k - 1 : 0], 0xff, 0xf, 0xf, true);
      lsd[k] = sub == 0 ? before : left;
      if (mine[k] && lsd[k] >= 0 && lsd[k] != sd[k]) cand = 4 * k + sub;
    }
    const int c = min(min(__builtin_amdgcn_update_dpp(0, cand, 0x00, 0xf, 0xf, true), __builtin_amdgcn_update_dpp(0, cand, 0x55, 0xf, 0xf, true)),
                      min(__builtin_amdgcn_update_dpp(0, cand, 0xaa, 0xf, 0xf, true), __builtin_amdgcn_update_dpp(0, cand, 0xff, 0xf, 0xf, true)));
    const bool found = c < 4 * K;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const bool walked = mine[k] && 4 * k + sub <= c;
      own += walked ? 1u : 0u;
      w.fetched += (walked && fetch[k]) ? 1u : 0u;
      w.skipped += (walked && !fetch[k]) ? 1u : 0u;
    }
    if (__ballot(found) != 0ull) { // (wave-uniform: the quad exchanges below run with every lane)
      const int kq = c >> 2, wl = c & 3;
      float t_at = tms[0], t_before = carry_tm;
      int s_at = sd[0], s_before = lsd[0];
#pragma unroll
      for (int k = 1; k < K; ++k) {
        const bool here = k == kq;
        t_at = here ? tms[k] : t_at;
        t_before = here ? tms[k - 1] : t_before; // (lane 3's: the predecessor of lane 0's step)
        s_at = here ? sd[k] : s_at;
        s_before = here ? lsd[k] : s_before;
      }
      const float tb = quad_pick(t_at, wl);
      const float ta_left = quad_pick(t_at, wl > 0 ? wl - 1 : 0), ta_carry = kq == 0 ? carry_tm : quad_bcast<3>(t_before);
      const float ta = wl > 0 ? ta_left : ta_carry;
      const int sb = quad_bcast_i(s_at, wl), sa = quad_bcast_i(s_before, wl);
      if (found) { w.hit = true; w.ta = ta; w.tb = tb; w.side_a = sa; w.side_b = sb; }
      if constexpr (RESUME) {
        float ty_at = tys[0];
#pragma unroll
        for (int k = 1; k < K; ++k) ty_at = k == kq ? tys[k] : ty_at;
        const float ty_hit = quad_pick(ty_at, wl);
        if (found) carry->ty = ty_hit;
      }
    }
    carry_side = __builtin_amdgcn_update_dpp(0, sd[K - 1], 0xff, 0xf, 0xf, true);
    carry_tm = quad_bcast<3>(tms[K - 1]);
    live = live && more && !found;
  }
  {
    const float o = __uint_as_float(own);
    w.steps = __float_as_uint(quad_bcast<0>(o)) + __float_as_uint(quad_bcast<1>(o)) + __float_as_uint(quad_bcast<2>(o)) + __float_as_uint(quad_bcast<3>(o));
  }
  return w;
}

struct IsoResult {
  bool hit;                                 // quad-uniform, like iso ... shadow
  float iso, t;                             // iso_{k*}, t*
  unsigned int steps;                       // steps walked
  f3 pos, n_w;                              // pos*, the world normal (SHADE >= 1)
  float shadow;                             // SHADE == 2: 1 iff the shadow ray crosses a level set
  unsigned int fetched, skipped, shadow_fetched, shadow_skipped; // THIS LANE's
};

// ---- translucent isosurfaces (include/ovr_hip.h ovr_hip_set_isosurface_layers; isosurface.py is the arithmetic).  The opaque path below
// (isosurface_ray without TRANS) is kept as it was, text and code: what the translucent ray shares with it - the refinement, the gradient taps - is restated here
// one crossing of a translucent ray
struct IsoPoint {
  float t;                                  // t* (quad-uniform, like pos ... shadow_steps)
  f3 pos, n_w;                              // pos*, the world normal (SHADE >= 1)
  float shadow;                             // SHADE == 2: the opacity the shadow ray accumulated
  unsigned int shadow_steps;                // the steps of its shadow walks
  unsigned int shadow_fetched, shadow_skipped; // THIS LANE's
};

// isovalue k and its opacity (k quad-uniform, 0 ... 3)
__device__ __forceinline__ float iso_value(const RayMarchParams& P, int ks)
{
  float iso = P.iso_values[0];
#pragma unroll
  for (int k = 1; k < kMaxIsovalues; ++k) iso = ks == k ? P.iso_values[k] : iso;
  return iso;
}
__device__ __forceinline__ float iso_opacity(const RayMarchParams& P, int ks)
{
  float a = P.iso_opacities[0];
#pragma unroll
  for (int k = 1; k < kMaxIsovalues; ++k) a = ks == k ? P.iso_opacities[k] : a;
  return a;
}
// the events of a step from side sa to side sb != sa, in the order the ray meets them: the first isovalue crossed and the direction
__device__ __forceinline__ void iso_step_events(int sa, int sb, int& k0, int& dk, int& n)
{
  const bool rising = sb > sa;
  k0 = rising ? sa : sa - 1; // rising: the lowest isovalue crossed first; falling: the highest
  dk = rising ? 1 : -1;
  n = rising ? sb - sa : sa - sb;
}

// one crossing of the level iso on the walk's pair (ta, tb) of the ray org + t dir: refined, and under SHADE >= 1 its normal, under SHADE == 2 its shadow term -
// by the opaque hit's operations.  hit: the quad has a crossing (the others tap along, clamped).  The shadow ray accumulates the opacities of the level sets it
// crosses, walk by walk, until it saturates
template <int VT, int AM, int SHADE, bool SKIP, bool CLIP>
__device__ __forceinline__ void iso_point(const RayMarchParams& P, const VolConsts& vc, const MarchConsts& mc, f3 org, f3 dir, float iso, float ta, float tb, bool hit,
                                          const SubMask& subm, IsoPoint& res)
{
  const int sub = subm.sub;
  auto tap_at = [&](float t) {
    const f3 p = mk3(fmaf(t, dir.x, org.x), fmaf(t, dir.y, org.y), fmaf(t, dir.z, org.z));
    return sample_volume<VT, AM>(vc, to_object(mc, p));
  };
  // the pair's samples: lanes 0 and 1, one instruction (the other two lanes repeat them)
  const float se = tap_at((sub & 1) ? tb : ta);
  float sa = quad_bcast<0>(se), sb = quad_bcast<1>(se);
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const float wd = tb - ta;
    const float p1 = fmaf(0.2f, wd, ta), p2 = fmaf(0.4f, wd, ta), p3 = fmaf(0.6f, wd, ta), p4 = fmaf(0.8f, wd, ta);
    const float q = tap_at(sel4(p1, p2, p3, p4, subm));
    const float q1 = quad_bcast<0>(q), q2 = quad_bcast<1>(q), q3 = quad_bcast<2>(q), q4 = quad_bcast<3>(q);
    const bool i0 = iso <= sa, i1 = iso <= q1, i2 = iso <= q2, i3 = iso <= q3, i4 = iso <= q4, i5 = iso <= sb;
    float nta = ta, nsa = sa, ntb = tb, nsb = sb; // (the last assignment that fires is the FIRST pair that differs)
    if (i4 != i5) { nta = p4; nsa = q4; ntb = tb; nsb = sb; }
    if (i3 != i4) { nta = p3; nsa = q3; ntb = p4; nsb = q4; }
    if (i2 != i3) { nta = p2; nsa = q2; ntb = p3; nsb = q3; }
    if (i1 != i2) { nta = p1; nsa = q1; ntb = p2; nsb = q2; }
    if (i0 != i1) { nta = ta; nsa = sa; ntb = p1; nsb = q1; }
    ta = nta; sa = nsa; tb = ntb; sb = nsb;
  }
  const float ts = fminf(fmaxf(fmaf((iso - sa) / (sb - sa), tb - ta, ta), ta), tb);
  res.t = ts;
  const f3 pos = mk3(fmaf(ts, dir.x, org.x), fmaf(ts, dir.y, org.y), fmaf(ts, dir.z, org.z));
  res.pos = pos;
  if (SHADE == 0) return;
  {
    // shade_request's forward difference: lane 0 taps s*, lanes 1 ... 3 the three neighbours - one instruction
    const f3 po = to_object(mc, pos);
    const bool flx = (po.x + mc.gstep.x) > 1.f, fly = (po.y + mc.gstep.y) > 1.f, flz = (po.z + mc.gstep.z) > 1.f;
    const float dx = flx ? -mc.gstep.x : mc.gstep.x, dy = fly ? -mc.gstep.y : mc.gstep.y, dz = flz ? -mc.gstep.z : mc.gstep.z;
    const f3 pg = mk3(sub == 1 ? po.x + dx : po.x, sub == 2 ? po.y + dy : po.y, sub == 3 ? po.z + dz : po.z);
    const float sg = sample_volume<VT, AM>(vc, pg);
    const float ss = quad_bcast<0>(sg), sgx = quad_bcast<1>(sg), sgy = quad_bcast<2>(sg), sgz = quad_bcast<3>(sg);
    f3 g;
#if OVR_PARITY_EXACT
    g.x = (sgx - ss) / dx; g.y = (sgy - ss) / dy; g.z = (sgz - ss) / dz;
#else
    g.x = (sgx - ss) * (flx ? -mc.ginv.x : mc.ginv.x);
    g.y = (sgy - ss) * (fly ? -mc.ginv.y : mc.ginv.y);
    g.z = (sgz - ss) * (flz ? -mc.ginv.z : mc.ginv.z);
#endif
    const f3 gn = normalize3(g);
    res.n_w = normalize3(mk3(-gn.x * mc.otw_it.x, -gn.y * mc.otw_it.y, -gn.z * mc.otw_it.z));
  }
  if (SHADE == 2) {
    // the hard shadow: the first crossing along pos* + t light from 1.5 steps on, nothing refined
    const f3 oo = to_object(mc, pos);
    const f3 od = mk3(mc.light.x * mc.inv_scale.x, mc.light.y * mc.inv_scale.y, mc.light.z * mc.inv_scale.z);
    float s0 = 0.f, s1 = FLT_MAX;
    const bool lit_ray = box_test<CLIP>(P, s0, s1, oo, od) && hit;
    {
      // the partial shadow: A_s = fma(1 - A_s, alpha_k, A_s) over the shadow ray's events, walk by walk, until it saturates.  Every pass of a ray that goes on
      // has consumed at least one of its steps: the loop is bounded by the ray's step count
      IsoCarry sc;
      sc.side = -1; sc.tm = 0.f; sc.ty = 0.f;
      float As = 0.f, stx = s0 + mc.step;
      bool go = lit_ray;
      while (__ballot(go) != 0ull) {
        const IsoWalk sw = iso_walk<VT, AM, SKIP, true>(P, vc, mc, pos, mc.light, stx, s1, go, subm, &sc);
        res.shadow_fetched += sw.fetched; res.shadow_skipped += sw.skipped; res.shadow_steps += sw.steps;
        if (sw.hit) {
          int k, dk, n;
          iso_step_events(sw.side_a, sw.side_b, k, dk, n);
#pragma unroll
          for (int e = 0; e < kMaxIsovalues; ++e) {
            if (e < n && !(As >= 0.9999f)) As = fmaf(1.f - As, iso_opacity(P, k), As);
            k += dk;
          }
        }
        go = sw.hit && !(As >= 0.9999f);
        stx = sc.ty; sc.side = sw.side_b; sc.tm = sw.tb;
      }
      res.shadow = As;
    }
  }
}

// a translucent ray (open-volume-renderer_amd/isosurface.py is the arithmetic)
struct IsoLayers {
  unsigned int events;                      // quad-uniform, like A ... shadow_steps: the events composited
  float A;                                  // the accumulated opacity
  float iso, t;                             // the first event's isovalue and t*: the layer
  unsigned int steps, shadow_steps;         // steps walked; the steps of all shadow walks
  unsigned int fetched, skipped, shadow_fetched, shadow_skipped; // THIS LANE's
};

// every crossing of the ray composited front to back until A >= 0.9999f or the ray leaves the box: walk - the events of the hit step, each behind a wave-uniform
// branch through iso_point - walk again from the hit step.  on_event(index, k, iso, alpha, tr = 1 - A before, A after, point) is called by the lanes of a quad
// that takes the event: the caller composites its colour there.  Both loops are bounded: a walk that hits has consumed at least one step of the ray, a step
// holds at most kMaxIsovalues events
template <int VT, int AM, int SHADE, bool SKIP, bool CLIP, class OnEvent>
__device__ __forceinline__ IsoLayers isosurface_layers(const RayMarchParams& P, const VolConsts& vc, const MarchConsts& mc, f3 org, f3 dir, float t0, float t1, bool live,
                                                       const SubMask& subm, OnEvent&& on_event)
{
  IsoLayers L;
  L.events = 0u; L.A = 0.f; L.iso = L.t = 0.f; L.steps = L.shadow_steps = 0u; L.fetched = L.skipped = L.shadow_fetched = L.shadow_skipped = 0u;
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
      if (__ballot(ev) == 0ull) break; // (wave-uniform: the quad exchanges of iso_point run with every lane)
      const float iso = iso_value(P, k), alpha = iso_opacity(P, k);
      IsoPoint pt;
      pt.t = 0.f; pt.pos = org; pt.n_w = mk3(0, 0, 0); pt.shadow = 0.f; pt.shadow_steps = pt.shadow_fetched = pt.shadow_skipped = 0u;
      iso_point<VT, AM, SHADE, SKIP, CLIP>(P, vc, mc, org, dir, iso, w.ta, w.tb, ev, subm, pt);
      L.shadow_fetched += pt.shadow_fetched; L.shadow_skipped += pt.shadow_skipped; // (a quad without the event walked no shadow step)
      if (ev) {
        const float tr = 1.f - L.A;
        const float A = fmaf(tr, alpha, L.A);
        on_event(L.events, k, iso, alpha, tr, A, pt);
        if (L.events == 0u) { L.iso = iso; L.t = pt.t; }
        L.A = A;
        ++L.events;
        L.shadow_steps += pt.shadow_steps;
        open = !(A >= 0.9999f);
      }
      k += dk;
    }
    go = w.hit && open;
    tx = carry.ty; carry.side = w.side_b; carry.tm = w.tb;
  }
  return L;
}

// the ray org + t dir (world space) over [t0, t1]; live: the ray is walked (quad-uniform)
template <int VT, int AM, int SHADE, bool SKIP, bool CLIP>
__device__ __forceinline__ IsoResult isosurface_ray(const RayMarchParams& P, const VolConsts& vc, const MarchConsts& mc, f3 org, f3 dir, float t0, float t1, bool live,
                                                    const SubMask& subm)
{
  static_assert(isosurface_variant_exists(SHADE, AM, SKIP, CLIP), "no such variant of the isosurface kernel (host/launch_plan.hpp)");
  const int sub = subm.sub;
  const IsoWalk w = iso_walk<VT, AM, SKIP>(P, vc, mc, org, dir, t0, t1, live, subm);
  IsoResult res;
  res.hit = w.hit; res.steps = w.steps; res.fetched = w.fetched; res.skipped = w.skipped;
  res.shadow = 0.f; res.shadow_fetched = res.shadow_skipped = 0u;
  res.n_w = mk3(0, 0, 0);
  // rising: the lowest isovalue crossed; falling: the highest
  const int ks = w.side_b > w.side_a ? w.side_a : w.side_a - 1;
  float iso = P.iso_values[0];
#pragma unroll
  for (int k = 1; k < kMaxIsovalues; ++k) iso = ks == k ? P.iso_values[k] : iso;
  res.iso = iso;
  res.t = 0.f; res.pos = org;
  if (__ballot(w.hit) == 0ull) return res; // (wave-uniform: nothing to refine or shade)
  auto tap_at = [&](float t) {
    const f3 p = mk3(fmaf(t, dir.x, org.x), fmaf(t, dir.y, org.y), fmaf(t, dir.z, org.z));
    return sample_volume<VT, AM>(vc, to_object(mc, p));
  };
  // the pair's samples: lanes 0 and 1, one instruction (the other two lanes repeat them)
  float ta = w.ta, tb = w.tb;
  const float se = tap_at((sub & 1) ? tb : ta);
  float sa = quad_bcast<0>(se), sb = quad_bcast<1>(se);
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const float wd = tb - ta;
    const float p1 = fmaf(0.2f, wd, ta), p2 = fmaf(0.4f, wd, ta), p3 = fmaf(0.6f, wd, ta), p4 = fmaf(0.8f, wd, ta);
    const float q = tap_at(sel4(p1, p2, p3, p4, subm));
    const float q1 = quad_bcast<0>(q), q2 = quad_bcast<1>(q), q3 = quad_bcast<2>(q), q4 = quad_bcast<3>(q);
    const bool i0 = iso <= sa, i1 = iso <= q1, i2 = iso <= q2, i3 = iso <= q3, i4 = iso <= q4, i5 = iso <= sb;
    float nta = ta, nsa = sa, ntb = tb, nsb = sb; // (the last assignment that fires is the FIRST pair that differs)
    if (i4 != i5) { nta = p4; nsa = q4; ntb = tb; nsb = sb; }
    if (i3 != i4) { nta = p3; nsa = q3; ntb = p4; nsb = q4; }
    if (i2 != i3) { nta = p2; nsa = q2; ntb = p3; nsb = q3; }
    if (i1 != i2) { nta = p1; nsa = q1; ntb = p2; nsb = q2; }
    if (i0 != i1) { nta = ta; nsa = sa; ntb = p1; nsb = q1; }
    ta = nta; sa = nsa; tb = ntb; sb = nsb;
  }
  const float ts = fminf(fmaxf(fmaf((iso - sa) / (sb - sa), tb - ta, ta), ta), tb);
  res.t = ts;
  const f3 pos = mk3(fmaf(ts, dir.x, org.x), fmaf(ts, dir.y, org.y), fmaf(ts, dir.z, org.z));
  res.pos = pos;
  if (SHADE == 0) return res;
  {
    // shade_request's forward difference: lane 0 taps s*, lanes 1 ... 3 the three neighbours - one instruction
    const f3 po = to_object(mc, pos);
    const bool flx = (po.x + mc.gstep.x) > 1.f, fly = (po.y + mc.gstep.y) > 1.f, flz = (po.z + mc.gstep.z) > 1.f;
    const float dx = flx ? -mc.gstep.x : mc.gstep.x, dy = fly ? -mc.gstep.y : mc.gstep.y, dz = flz ? -mc.gstep.z : mc.gstep.z;
    const f3 pg = mk3(sub == 1 ? po.x + dx : po.x, sub == 2 ? po.y + dy : po.y, sub == 3 ? po.z + dz : po.z);
    const float sg = sample_volume<VT, AM>(vc, pg);
    const float ss = quad_bcast<0>(sg), sgx = quad_bcast<1>(sg), sgy = quad_bcast<2>(sg), sgz = quad_bcast<3>(sg);
    f3 g;
#if OVR_PARITY_EXACT
    g.x = (sgx - ss) / dx; g.y = (sgy - ss) / dy; g.z = (sgz - ss) / dz;
#else
    g.x = (sgx - ss) * (flx ? -mc.ginv.x : mc.ginv.x);
    g.y = (sgy - ss) * (fly ? -mc.ginv.y : mc.ginv.y);
    g.z = (sgz - ss) * (flz ? -mc.ginv.z : mc.ginv.z);
#endif
    const f3 gn = normalize3(g);
    res.n_w = normalize3(mk3(-gn.x * mc.otw_it.x, -gn.y * mc.otw_it.y, -gn.z * mc.otw_it.z));
  }
  if (SHADE == 2) {
    // the hard shadow: the first crossing along pos* + t light from 1.5 steps on, nothing refined
    const f3 oo = to_object(mc, pos);
    const f3 od = mk3(mc.light.x * mc.inv_scale.x, mc.light.y * mc.inv_scale.y, mc.light.z * mc.inv_scale.z);
    float s0 = 0.f, s1 = FLT_MAX;
    const bool lit_ray = box_test<CLIP>(P, s0, s1, oo, od) && w.hit;
    const IsoWalk sw = iso_walk<VT, AM, SKIP>(P, vc, mc, pos, mc.light, s0 + mc.step, s1, lit_ray, subm);
    res.shadow = sw.hit ? 1.f : 0.f;
    res.shadow_fetched = sw.fetched; res.shadow_skipped = sw.skipped;
  }
  return res;
}
// TRANS (an overload: the opaque function above is what it was, text and code): the translucent ray - an IsoLayers, and on_event per composited event
template <int VT, int AM, int SHADE, bool SKIP, bool CLIP, bool TRANS, class OnEvent>
__device__ __forceinline__ IsoLayers isosurface_ray(const RayMarchParams& P, const VolConsts& vc, const MarchConsts& mc, f3 org, f3 dir, float t0, float t1, bool live,
                                                    const SubMask& subm, OnEvent&& on_event)
{
  static_assert(TRANS && isosurface_variant_exists(SHADE, AM, SKIP, CLIP, false, TRANS), "no such variant of the isosurface kernel (host/launch_plan.hpp)");
  return isosurface_layers<VT, AM, SHADE, SKIP, CLIP>(P, vc, mc, org, dir, t0, t1, live, subm, on_event);
}

// the colour of an isovalue, once per hit, from the table in global memory: project_classify's colour half (the alpha table is not read)
__device__ __forceinline__ f3 isosurface_colour(const RayMarchParams& P, float v)
{
  const float c = clamp01((fminf(fmaxf(v, P.tf_lower), P.tf_upper) - P.tf_lower) * P.tf_scale);
  const int nc1 = P.n_color - 1;
  const float xc = c * (float)nc1;
  const int ic = (int)xc;
  const float fc = __builtin_amdgcn_fractf(xc);
  const float4* col = reinterpret_cast<const float4*>(P.tf_color);
  const float4 a = col[ic], b = col[min(ic + 1, nc1)];
  return mk3(clamp01(lerpf(a.x, b.x, fc)), clamp01(lerpf(a.y, b.y, fc)), clamp01(lerpf(a.z, b.z, fc)));
}

// an isosurface frame: project_kernel's frame around isosurface_ray; the layer is (iso, t*, 1).  The material is a run-time argument (shade_light<true> with
// the reference's values IS the reference's expression, operation for operation): one instantiation per shading mode, none per material
// ORTHO: the orthographic camera's rays (pixel_ray) and view vector (shade_light) - on the clipped variants alone
// TRANS: the translucent frame - every crossing composited, the pixel un-premultiplied like the march's - on the clipped variants alone
template <int VT, int AM, int SHADE, bool SKIP, bool CLIP, bool ORTHO = false, bool TRANS = false>
__global__ __launch_bounds__(kBlock) void isosurface_kernel(const RayMarchParams P)
{
  static_assert(isosurface_variant_exists(SHADE, AM, SKIP, CLIP, ORTHO, TRANS) && (AM != 4 || RowLoads<VT, 4>::on), "no such variant of the isosurface kernel (host/launch_plan.hpp)");
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
    if constexpr (TRANS) {
      // the colour lookup and the shade factor in front of the composite: C_ch = fma(tr * c_ch, alpha, C_ch), the march's expression
      f3 cc = mk3(0, 0, 0);
      auto on_event = [&](unsigned int, int, float iso, float alpha, float tr, float, const IsoPoint& pt) {
        if (!owner) return;
        f3 c = isosurface_colour(P, iso);
        if (SHADE != 0) {
          const float shade = shade_factor<true>(P, shade_light<true, ORTHO>(P, mc.light, pt.n_w, pt.pos), pt.shadow);
          c = mk3(clamp01(c.x * shade), clamp01(c.y * shade), clamp01(c.z * shade));
        }
        cc.x = fmaf(tr * c.x, alpha, cc.x); cc.y = fmaf(tr * c.y, alpha, cc.y); cc.z = fmaf(tr * c.z, alpha, cc.z);
      };
      const IsoLayers il = isosurface_ray<VT, AM, SHADE, SKIP, CLIP, true>(P, vc, mc, org, dir, t0, t1, live, subm, on_event);
      n_samples += il.fetched;
      n_skipped += il.skipped;
      n_shadow += il.shadow_fetched;
      n_shadow_skipped += il.shadow_skipped;
      if (il.events > 0u && owner) {
        n_hits += il.events;
        o_c.x += cc.x / il.A; o_c.y += cc.y / il.A; o_c.z += cc.z / il.A;
        o_a += il.A;
        o_g.x += il.iso; o_g.y += il.t; o_g.z += 1.f;
      }
    }
    else {
      const IsoResult ir = isosurface_ray<VT, AM, SHADE, SKIP, CLIP>(P, vc, mc, org, dir, t0, t1, live, subm);
      n_samples += ir.fetched;
      n_skipped += ir.skipped;
      n_shadow += ir.shadow_fetched;
      n_shadow_skipped += ir.shadow_skipped;
      if (ir.hit && owner) {
        f3 c = isosurface_colour(P, ir.iso);
        if (SHADE != 0) {
          const float shade = shade_factor<true>(P, shade_light<true, ORTHO>(P, mc.light, ir.n_w, ir.pos), ir.shadow);
          c = mk3(clamp01(c.x * shade), clamp01(c.y * shade), clamp01(c.z * shade));
        }
        ++n_hits;
        o_c.x += c.x; o_c.y += c.y; o_c.z += c.z;
        o_a += 1.f;
        o_g.x += ir.iso; o_g.y += ir.t; o_g.z += 1.f;
      }
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

// the known-answer entry's kernel: ray i = the quad of lanes 4 i ... 4 i + 3, through isosurface_ray as the frame's kernel calls it with full shading (the normal
// and the shadow term are always computed).  The clipped box test alone: the bounds (0, 1) without a clip box give the unclipped test's bits
template <int VT, int AM, bool SKIP>
__global__ __launch_bounds__(kBlock) void isosurface_floats_kernel(const RayMarchParams P, const float* org, const float* dir, float* out, long long n)
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
  const IsoResult ir = isosurface_ray<VT, AM, 2, SKIP, true>(P, vc, mc, o, d, t0, t1, live, subm);
  if (valid && sub == 0) {
    float* q = out + 8 * i;
    q[0] = ir.hit ? 1.f : 0.f; q[1] = ir.hit ? ir.iso : 0.f; q[2] = ir.hit ? ir.t : 0.f; q[3] = live ? (float)ir.steps : 0.f;
    q[4] = ir.hit ? ir.n_w.x : 0.f; q[5] = ir.hit ? ir.n_w.y : 0.f; q[6] = ir.hit ? ir.n_w.z : 0.f; q[7] = ir.hit ? ir.shadow : 0.f;
  }
}

// its translucent twin (ovr_hip_isosurface_layers_floats): ray i through isosurface_ray<TRANS> as the translucent frame's kernel calls it with full shading ->
// 4 + 8 max_events floats: (events composited, A, steps walked, shadow steps over all events), then per event e < min(events, max_events)
// (k, t*, n_w.x, n_w.y, n_w.z, shadow, A after the event, 0).  The host zeroes `out` first: the rest stays zero
template <int VT, int AM, bool SKIP>
__global__ __launch_bounds__(kBlock) void isosurface_layers_floats_kernel(const RayMarchParams P, const float* org, const float* dir, float* out, long long n, int max_events)
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
  float* q = out + (4 + 8 * (long long)max_events) * j;
  auto on_event = [&](unsigned int e, int k, float, float, float, float A, const IsoPoint& pt) {
    if (sub != 0 || e >= (unsigned int)max_events) return; // (called by live quads alone: valid holds)
    float* p = q + 4 + 8 * e;
    p[0] = (float)k; p[1] = pt.t; p[2] = pt.n_w.x; p[3] = pt.n_w.y; p[4] = pt.n_w.z; p[5] = pt.shadow; p[6] = A; p[7] = 0.f;
  };
  const IsoLayers il = isosurface_ray<VT, AM, 2, SKIP, true, true>(P, vc, mc, o, d, t0, t1, live, subm, on_event);
  if (valid && sub == 0) { q[0] = (float)il.events; q[1] = il.A; q[2] = live ? (float)il.steps : 0.f; q[3] = (float)il.shadow_steps; }
}

// the isosurface kernels of a voxel type, TRANS: the translucent ones - ONE LOOKUP, TWO EXPLICIT INSTANTIATIONS PER TYPE, each in an object
// of its own (ovr_hip_isosurface.hip without and with -DOVR_ISO_LAYERS): beside the translucent kernels the opaque ones took other registers, so the opaque
// kernels' object is compiled from what it was compiled from.  The translucent kernels exist on the clipped box test alone (isosurface_variant_exists)
typedef void (*IsosurfaceFloatsKernel)(const RayMarchParams, const float*, const float*, float*, long long);
typedef void (*IsosurfaceLayersFloatsKernel)(const RayMarchParams, const float*, const float*, float*, long long, int);
template <bool TRANS> struct IsosurfaceKernelsOf { // nullptr: no such variant of this type
  FrameKernel frame = nullptr;
  std::conditional_t<TRANS, IsosurfaceLayersFloatsKernel, IsosurfaceFloatsKernel> floats = nullptr;
};
typedef IsosurfaceKernelsOf<false> IsosurfaceKernels;
typedef IsosurfaceKernelsOf<true> IsosurfaceLayersKernels;
template <int VT, int AM, bool TRANS> struct IsosurfaceVariants {
  template <unsigned I> static constexpr IsosurfaceKernelsOf<TRANS> at()
  {
    constexpr int shade = (int)(I / kWalkBitsEnd);
    constexpr bool skip = I & kWalkSkip, clipped = I & kWalkClipped, ortho = I & kWalkOrtho;
    if constexpr (!isosurface_variant_exists(shade, AM, skip, clipped, ortho, TRANS)) return {};
    else if constexpr (TRANS) return { isosurface_kernel<VT, AM, shade, skip, clipped, ortho, true>, isosurface_layers_floats_kernel<VT, AM, skip> };
    else return { isosurface_kernel<VT, AM, shade, skip, clipped, ortho>, isosurface_floats_kernel<VT, AM, skip> };
  }
};
// an isosurface plan's kernels of a voxel type - the opaque ones for an opaque plan, the translucent ones for a translucent plan; nullptr otherwise, for a
// replica's type and for mode 4 on a layout without row loads, like project_kernels_of
template <int VT, bool TRANS>
IsosurfaceKernelsOf<TRANS> isosurface_kernels_of(const LaunchPlan& pl)
{
  constexpr unsigned n = 3 * kWalkBitsEnd;
  const unsigned i = (unsigned)pl.shading * kWalkBitsEnd + walk_bits(pl.isosurface.skip, pl.isosurface.clipped, pl.orthographic);
  if (pl.error || !pl.isosurface.on || pl.isosurface.translucent != TRANS || i >= n) return IsosurfaceKernelsOf<TRANS>();
  return dispatch_addressing<IsosurfaceKernelsOf<TRANS>, VT, true>(pl.am, [&](auto m) {
    return variant_at<IsosurfaceVariants<VT, decltype(m)::value, TRANS>>(i, std::make_integer_sequence<unsigned, n>());
  });
}

// one explicit instantiation per voxel type, each an object of its own (ovr_hip_march.hip, compiled once per type): the ~160 kernel
// variants of a type compile in parallel with the other types
template <int VT>
FrameKernels frame_kernels(const LaunchPlan& pl)
{
  const unsigned flags = (pl.skip ? kBitSkip : 0u) | (pl.pooled ? kBitPooled : 0u) | (pl.march.lds_staged ? kBitLdsStaged : 0u) | (pl.march.deep ? kBitDeep : 0u);
  const unsigned ortho = pl.orthographic ? kBitOrtho : 0u;
  const unsigned march_bits = flags | (pl.march.material ? kBitMaterial : 0u) | (pl.march.clipped ? kBitClipped : 0u) | (pl.cached && !pl.pooled ? kBitCached : 0u) | ortho;
  const unsigned shade_bits = (flags & kBitSkip) | (pl.shade.material ? kBitMaterial : 0u) | (pl.shade.clipped ? kBitClipped : 0u) | (pl.cached ? kBitCached : 0u) | ortho;
  FrameKernels k;
  if (pl.error) return k;
  switch (pl.shading) {
  case 0: k = variants_of<VT, 0>(pl.am, march_bits, shade_bits); break;
  case 1: k = variants_of<VT, 1>(pl.am, march_bits, shade_bits); break;
  case 2: k = variants_of<VT, 2>(pl.am, march_bits, shade_bits); break;
  }
  if (!pl.pooled) k.shade = nullptr;
  return k;
}

} // namespace ovrhip
