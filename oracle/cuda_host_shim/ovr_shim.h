// ovr_shim.h - what the driver of the host-compiled marcher (oracle/ref_march_probe.cpp) tells the shim: textures, the one
// instance of the scene, the launch index; and what it reads back: iteration counters.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <cstdint>

// A texture object of the shim is the address of one of these.  The texture is always the one kind the reference creates
// (normalised coordinates, clamp addressing, linear filter); `format` says how a texel becomes a float.
enum OvrShimFormat {
  OVR_SHIM_F32 = 0, // element read
  OVR_SHIM_U8,      // normalised read: v / 255
  OVR_SHIM_I8,      // normalised read: max(v / 127, -1)
  OVR_SHIM_U32,     // the reference asks CUDA for a normalised read of 32-bit integers, which CUDA does not define
  OVR_SHIM_I32,     // (cudaReadModeNormalizedFloat is for 8- and 16-bit integers): restated as the reference's integer_normalize
  OVR_SHIM_F32X4,   // float4 element read
};
struct OvrShimTexture {
  const void* data;
  int format;
  int dims[3]; // x fastest; unused trailing dimensions are 1
};

// the scene: one instance of one custom-primitive (AABB [0,1]^3) geometry.  object_to_world is the 3x4 row-major instance
// transform; sbt_data is what optixGetSbtDataPointer() returns in the instance's hit programs.
void ovr_shim_set_instance(const float object_to_world[12], const void* sbt_data, unsigned visibility_mask);
// the shader binding table: one hit group (intersection + closest-hit program) and one miss program per ray type.  optixTrace picks
// hit group `sbt_offset + sbt_stride * 0 + instance offset 0` and miss program `miss_index` (OptiX Programming Guide, "Shader
// binding table", "SBT instance offset / geometry-AS index").
typedef void (*OvrShimProgram)();
void ovr_shim_set_programs(int ray_types, const OvrShimProgram* intersection, const OvrShimProgram* closest_hit, const OvrShimProgram* miss);
void ovr_shim_set_launch_index(unsigned x, unsigned y);
// out[0]: colour-table fetches outside a shadow-ray trace (= iterations of the primary march); out[1]: inside one
void ovr_shim_get_counters(uint64_t out[2]);
void ovr_shim_reset_counters();
// 0 (default): exact float filter weights.  n > 0: the fractional part of every filter coordinate is rounded to n bits first
// (CUDA hardware keeps 8, Programming Guide "Linear Filtering") - for a report, not for the fixture.
void ovr_shim_set_filter_fraction_bits(int n);
