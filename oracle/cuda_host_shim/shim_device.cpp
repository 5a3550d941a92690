// shim_device.cpp - definitions of the device-side names the reference's ray marcher executes when it is compiled for the host
// (see cuda_runtime.h).  TEST INFRASTRUCTURE ONLY.  Every function states the documented rule it follows.  This file is compiled
// ONCE per build with -ffp-contract=off and without -mfma, whatever the marcher's own flags are: texture filtering, the ray
// transform and __powf are not code that nvcc compiles, so the freedom the two probe builds bracket (where nvcc contracts a * b + c
// of the shader text) must not reach into them.
//
// Not reproduced, by construction: the hardware's 8-bit filter weights (ovr_shim_set_filter_fraction_bits reports their size),
// ex2.approx / lg2.approx behind __powf, OptiX's own arithmetic for the inverse instance transform and the ray transform.
#include "cuda_runtime.h"
#include "ovr_shim.h"

#include <cstdlib>

// ---------------------------------------------------------------------------------------------------------------------------------
// intrinsics
// ---------------------------------------------------------------------------------------------------------------------------------
// CUDA Math API: __frcp_rn "compute 1/x in round-to-nearest-even mode" - IEEE division is that.
float __frcp_rn(float x) { return 1.f / x; }
// CUDA Programming Guide, "Intrinsic Functions": __powf(x, y) is implemented as exp2f(y * __log2f(x)).  The structure is kept
// (log2, one float product, exp2); the two approximate instructions are replaced by libm's functions.
float ovr_shim_powf(float x, float y)
{
  const float l = log2f(x);
  const float m = y * l;
  return exp2f(m);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// texture fetches - CUDA Programming Guide, appendix "Texture Fetching":
//   normalised coordinate x in [0, 1] -> x * N                       ("x is replaced by ... N x")
//   clamp addressing: the texel index is clamped to [0, N - 1]
//   linear filtering: xB = x - 0.5, i = floor(xB), alpha = frac(xB),
//     1D: tex(x) = (1 - alpha) T[i] + alpha T[i + 1]
//     3D: tex(x, y, z) = (1-a)(1-b)(1-c) T[i,j,k] + a(1-b)(1-c) T[i+1,j,k] + (1-a)b(1-c) T[i,j+1,k] + ab(1-c) T[i+1,j+1,k]
//                      + (1-a)(1-b)c T[i,j,k+1] + a(1-b)c T[i+1,j,k+1] + (1-a)bc T[i,j+1,k+1] + abc T[i+1,j+1,k+1]
//   The hardware stores alpha, beta, gamma in 9-bit fixed point with 8 fractional bits, so its eight weights sum to exactly one and a
//   region of equal texels filters to exactly that value (the marcher's finite-difference gradient is then exactly zero there and its
//   normal NaN, which the shader's clamp drops).  Summing the eight float products above loses that: the weights no longer sum to one
//   and a constant region returns its value times 1 +- 1e-7, which the gradient amplifies into a normal of random direction.  The
//   default here keeps alpha, beta, gamma as exact floats but evaluates the same polynomial as nested interpolations
//   T0 + w * (T1 - T0), along x, then y, then z, each product and sum rounded to float: exact on equal texels, like the hardware.
// ---------------------------------------------------------------------------------------------------------------------------------
static int g_fraction_bits = 0;
void ovr_shim_set_filter_fraction_bits(int n) { g_fraction_bits = n; }

namespace {

struct Axis { int i0, i1; float w; };

inline Axis filter_axis(float x, int n)
{
  const float xn = x * (float)n;
  const float xb = xn - 0.5f;
  const float fl = floorf(xb);
  float w = xb - fl;
  if (g_fraction_bits > 0) {
    const float q = (float)(1 << g_fraction_bits);
    w = rintf(w * q) / q; // may reach 1: then the fetch returns T[i + 1], as a weight of 256/256 does
  }
  int i0 = (int)fl, i1 = (int)fl + 1;
  i0 = i0 < 0 ? 0 : (i0 > n - 1 ? n - 1 : i0);
  i1 = i1 < 0 ? 0 : (i1 > n - 1 ? n - 1 : i1);
  return { i0, i1, w };
}

// one texel as the float a fetch filters: the element for float data; for integers the normalised value.  8-bit: Programming
// Guide, "Texture Object API", cudaReadModeNormalizedFloat: unsigned 8-bit -> [0, 1] (v / 255), signed 8-bit -> [-1, 1] (v / 127, the
// most negative value clamped).  32-bit integers: CUDA defines no normalised read; the value is what the reference's own
// integer_normalize<float, T> gives (static_cast<float>(v) / static_cast<float>(max), signed clamped at -1).
inline float texel(const OvrShimTexture* t, size_t idx)
{
  switch (t->format) {
  case OVR_SHIM_F32: return ((const float*)t->data)[idx];
  case OVR_SHIM_U8: return (float)((const uint8_t*)t->data)[idx] / 255.f;
  case OVR_SHIM_I8: { const float n = (float)((const int8_t*)t->data)[idx] / 127.f; return n < -1.f ? -1.f : n; }
  case OVR_SHIM_U32: return (float)((const uint32_t*)t->data)[idx] / (float)UINT32_MAX;
  case OVR_SHIM_I32: { const float n = (float)((const int32_t*)t->data)[idx] / (float)INT32_MAX; return n < -1.f ? -1.f : n; }
  default: fprintf(stderr, "[ovr_shim] scalar fetch from a texture of format %d\n", t->format); abort();
  }
}

inline float mix(float t0, float t1, float w) { return t0 + w * (t1 - t0); }

thread_local int t_trace_depth = 0;
uint64_t g_counters[2] = { 0, 0 };

} // namespace

void ovr_shim_get_counters(uint64_t out[2]) { out[0] = g_counters[0]; out[1] = g_counters[1]; }
void ovr_shim_reset_counters() { g_counters[0] = g_counters[1] = 0; }

template<> float tex1D<float>(cudaTextureObject_t tex, float x)
{
  const OvrShimTexture* t = (const OvrShimTexture*)tex;
  const Axis a = filter_axis(x, t->dims[0]);
  return mix(texel(t, (size_t)a.i0), texel(t, (size_t)a.i1), a.w);
}

template<> float4 tex1D<float4>(cudaTextureObject_t tex, float x)
{
  const OvrShimTexture* t = (const OvrShimTexture*)tex;
  if (t->format != OVR_SHIM_F32X4) { fprintf(stderr, "[ovr_shim] float4 fetch from a texture of format %d\n", t->format); abort(); }
  // the marcher fetches the colour table exactly once per iteration of either march: outside any nested trace that is an
  // iteration of the primary march, inside one (a trace started from a hit program) an iteration of the shadow march
  g_counters[t_trace_depth >= 2 ? 1 : 0]++;
  const Axis a = filter_axis(x, t->dims[0]);
  const float4* d = (const float4*)t->data;
  const float4 p = d[a.i0], q = d[a.i1];
  return make_float4(mix(p.x, q.x, a.w), mix(p.y, q.y, a.w), mix(p.z, q.z, a.w), mix(p.w, q.w, a.w));
}

template<> float tex3D<float>(cudaTextureObject_t tex, float x, float y, float z)
{
  const OvrShimTexture* t = (const OvrShimTexture*)tex;
  const Axis a = filter_axis(x, t->dims[0]), b = filter_axis(y, t->dims[1]), c = filter_axis(z, t->dims[2]);
  const size_t nx = (size_t)t->dims[0], ny = (size_t)t->dims[1];
#define T3(i, j, k) texel(t, (size_t)(i) + nx * ((size_t)(j) + ny * (size_t)(k)))
  const float c00 = mix(T3(a.i0, b.i0, c.i0), T3(a.i1, b.i0, c.i0), a.w), c10 = mix(T3(a.i0, b.i1, c.i0), T3(a.i1, b.i1, c.i0), a.w);
  const float c01 = mix(T3(a.i0, b.i0, c.i1), T3(a.i1, b.i0, c.i1), a.w), c11 = mix(T3(a.i0, b.i1, c.i1), T3(a.i1, b.i1, c.i1), a.w);
  return mix(mix(c00, c10, b.w), mix(c01, c11, b.w), c.w);
#undef T3
}

// ---------------------------------------------------------------------------------------------------------------------------------
// OptiX: one instance of one custom primitive, no any-hit programs.  Rules relied on (OptiX 7 Programming Guide):
//   * "Instance acceleration structures" / OptixInstance::visibilityMask with "Ray information" / optixTrace: an instance is
//     visited iff (ray visibility mask & instance visibility mask) != 0; only the 8 low bits of either count.
//   * "Transformations": the ray is transformed into the instance's object space with the inverse of the instance transform;
//     origin as a point, direction as a vector, NOT re-normalised, so t means the same in both spaces
//     (optixGetObjectRayOrigin / Direction vs. optixGetWorldRayOrigin / Direction).
//   * "Intersection program" / optixReportIntersection: a reported t is accepted iff it lies in [tmin, current tmax]; on
//     acceptance (no any-hit program, so nothing can reject it) the current tmax becomes t and the attributes are recorded.
//     optixGetRayTmax: "in intersection and closest-hit programs ... the current smallest reported hitT or the tmax passed into
//     optixTrace if no hit has been reported"; in a miss program the tmax passed into optixTrace.
//   * "Closest-hit / miss": after traversal the closest-hit program of hit group (sbt_offset + sbt_stride * geometry index 0 +
//     instance sbtOffset 0) runs if a hit was accepted, else miss program `miss_index`.  optixGetAttribute_n, the transform
//     matrices (3x4 row-major) and optixGetSbtDataPointer refer to the accepted hit; the payload registers are shared by reference.
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

struct Instance {
  float otw[12], wto[12];
  const void* sbt_data = nullptr;
  unsigned mask = 0;
} g_instance;

struct Programs {
  int ray_types = 0;
  OvrShimProgram intersection[4], closest_hit[4], miss[4];
} g_programs;

struct TraceRecord {
  float3 world_org, world_dir, object_org, object_dir;
  float tmin, tmax;
  unsigned mask;
  unsigned *p0, *p1;
  unsigned a0 = 0, a1 = 0;
  bool hit = false;
};

thread_local TraceRecord* t_current = nullptr;
thread_local uint3 t_launch_index = { 0, 0, 0 };

inline const TraceRecord& current()
{
  if (!t_current) { fprintf(stderr, "[ovr_shim] an optixGet* accessor was called outside optixTrace\n"); abort(); }
  return *t_current;
}

} // namespace

void ovr_shim_set_instance(const float object_to_world[12], const void* sbt_data, unsigned visibility_mask)
{
  memcpy(g_instance.otw, object_to_world, sizeof(g_instance.otw));
  // inverse of the affine transform, evaluated in double and rounded once per entry: OptiX does not document its arithmetic
  const float* m = object_to_world;
  const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
  const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
  const double inv[9] = { (e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det, (f * g - d * i) / det, (a * i - c * g) / det,
                          (c * d - a * f) / det, (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det };
  const double p[3] = { m[3], m[7], m[11] };
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) g_instance.wto[4 * r + k] = (float)inv[3 * r + k];
    g_instance.wto[4 * r + 3] = (float)-(inv[3 * r] * p[0] + inv[3 * r + 1] * p[1] + inv[3 * r + 2] * p[2]);
  }
  g_instance.sbt_data = sbt_data;
  g_instance.mask = visibility_mask & 0xffu;
}

void ovr_shim_set_programs(int ray_types, const OvrShimProgram* intersection, const OvrShimProgram* closest_hit, const OvrShimProgram* miss)
{
  if (ray_types < 1 || ray_types > 4) { fprintf(stderr, "[ovr_shim] %d ray types\n", ray_types); abort(); }
  g_programs.ray_types = ray_types;
  for (int k = 0; k < ray_types; ++k) {
    g_programs.intersection[k] = intersection[k];
    g_programs.closest_hit[k] = closest_hit[k];
    g_programs.miss[k] = miss[k];
  }
}

void ovr_shim_set_launch_index(unsigned x, unsigned y) { t_launch_index = make_uint3(x, y, 0); }
uint3 optixGetLaunchIndex() { return t_launch_index; }

void optixTrace(OptixTraversableHandle, float3 origin, float3 direction, float tmin, float tmax, float /*time*/, OptixVisibilityMask mask,
                unsigned /*flags: any-hit is disabled and there is none*/, unsigned sbt_offset, unsigned /*sbt_stride: geometry index 0*/,
                unsigned miss_index, unsigned& p0, unsigned& p1)
{
  if ((int)sbt_offset >= g_programs.ray_types || (int)miss_index >= g_programs.ray_types) { fprintf(stderr, "[ovr_shim] SBT index out of range\n"); abort(); }
  TraceRecord rec;
  rec.world_org = origin;
  rec.world_dir = direction;
  const float* w = g_instance.wto;
  rec.object_org = make_float3(w[0] * origin.x + w[1] * origin.y + w[2] * origin.z + w[3], w[4] * origin.x + w[5] * origin.y + w[6] * origin.z + w[7],
                               w[8] * origin.x + w[9] * origin.y + w[10] * origin.z + w[11]);
  rec.object_dir = make_float3(w[0] * direction.x + w[1] * direction.y + w[2] * direction.z, w[4] * direction.x + w[5] * direction.y + w[6] * direction.z,
                               w[8] * direction.x + w[9] * direction.y + w[10] * direction.z);
  rec.tmin = tmin;
  rec.tmax = tmax;
  rec.mask = mask & 0xffu;
  rec.p0 = &p0;
  rec.p1 = &p1;
  TraceRecord* const outer = t_current;
  t_current = &rec;
  ++t_trace_depth;
  if (rec.mask & g_instance.mask) g_programs.intersection[sbt_offset]();
  if (rec.hit)
    g_programs.closest_hit[sbt_offset]();
  else
    g_programs.miss[miss_index]();
  --t_trace_depth;
  t_current = outer;
}

bool optixReportIntersection(float t, unsigned /*kind*/, unsigned a0, unsigned a1)
{
  TraceRecord& r = *t_current;
  if (!(t >= r.tmin && t <= r.tmax)) return false;
  r.tmax = t;
  r.a0 = a0;
  r.a1 = a1;
  r.hit = true;
  return true;
}

float optixGetRayTmin() { return current().tmin; }
float optixGetRayTmax() { return current().tmax; }
float3 optixGetWorldRayOrigin() { return current().world_org; }
float3 optixGetWorldRayDirection() { return current().world_dir; }
float3 optixGetObjectRayOrigin() { return current().object_org; }
float3 optixGetObjectRayDirection() { return current().object_dir; }
unsigned optixGetPayload_0() { return *current().p0; }
unsigned optixGetPayload_1() { return *current().p1; }
unsigned optixGetAttribute_0() { return current().a0; }
unsigned optixGetAttribute_1() { return current().a1; }
unsigned optixGetRayVisibilityMask() { return current().mask; }
CUdeviceptr optixGetSbtDataPointer() { return (CUdeviceptr)g_instance.sbt_data; }
void optixGetWorldToObjectTransformMatrix(float m[12]) { memcpy(m, g_instance.wto, sizeof(g_instance.wto)); }
void optixGetObjectToWorldTransformMatrix(float m[12]) { memcpy(m, g_instance.otw, sizeof(g_instance.otw)); }
