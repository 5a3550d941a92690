// slices_host.hpp - the host arithmetic of ovr_hip_set_slices (include/ovr_hip.h; open-volume-renderer_amd/slices.py `commit` is the same in numpy): what the
// caller's point, normal, thickness and mode become, and which values are refused.  Nothing here calls HIP or knows the renderer:
// tests/slices_host_driver.cpp holds it to literals on a machine without a GPU, under the address and undefined-behaviour sanitizers.
#pragma once

#include <cmath>

namespace ovrhip {
namespace host {

struct SliceValues { float normal[3]; float c; };

// n = the normal normalised in float64, each component rounded to float32; c = dot(n, point) formed in float64 from the ROUNDED n and rounded once.
// Returns nullptr, or why the slice is refused (EINVAL): a non-finite point; a normal that is zero, non-finite or not normalisable (its float64 length is 0 or
// overflows, or a rounded component is not finite, or every rounded component is 0); a NaN or negative thickness; with thickness > 0 a mode outside 1 ... 3
inline const char* slice_values(const float point[3], const float normal[3], float thickness, int mode, SliceValues* out)
{
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(point[a])) return "a slice's point must be finite";
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(normal[a])) return "a slice's normal must be finite";
  const double x = normal[0], y = normal[1], z = normal[2];
  const double len = std::sqrt(x * x + y * y + z * z);
  if (!(len > 0.0) || !std::isfinite(len)) return "a slice's normal cannot be normalised";
  SliceValues v;
  v.normal[0] = (float)(x / len); v.normal[1] = (float)(y / len); v.normal[2] = (float)(z / len);
  if (!std::isfinite(v.normal[0]) || !std::isfinite(v.normal[1]) || !std::isfinite(v.normal[2]) || (v.normal[0] == 0.f && v.normal[1] == 0.f && v.normal[2] == 0.f))
    return "a slice's normal cannot be normalised";
  if (!(thickness >= 0.f)) return "a slice's thickness is 0, positive or +inf";
  if (thickness > 0.f && (mode < 1 || mode > 3)) return "a slab's mode is OVR_HIP_PROJECT_MAXIMUM, MINIMUM or MEAN";
  v.c = (float)((double)v.normal[0] * (double)point[0] + (double)v.normal[1] * (double)point[1] + (double)v.normal[2] * (double)point[2]);
  if (out) *out = v;
  return nullptr;
}

} // namespace host
} // namespace ovrhip
