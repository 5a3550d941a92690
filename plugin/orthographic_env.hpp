// orthographic_env.hpp - OVR_HIP_ORTHOGRAPHIC as data: "<height>" or "auto".  Pure (no HIP, no plugin state), so that tests/test_camera_plan.py can hold it to
// a table on a machine without a GPU.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstring>

namespace ovrhip_plugin {

enum { kOrthographicError = -1, kOrthographicHeight = 1, kOrthographicAuto = 2 };

// "auto" -> kOrthographicAuto; one finite float > 0 with the whole string consumed -> kOrthographicHeight and *height; anything else (an empty string, trailing
// text, a second value, zero, a negative or non-finite number, another word) -> kOrthographicError - an error, never another camera than the user wrote
inline int parse_orthographic(const char* text, float* height)
{
  if (!text || !*text) return kOrthographicError;
  if (std::strcmp(text, "auto") == 0) return kOrthographicAuto;
  float h = 0.f;
  int used = 0;
  if (std::sscanf(text, "%f%n", &h, &used) != 1 || used <= 0 || text[used] != 0) return kOrthographicError;
  if (!std::isfinite(h) || !(h > 0.f)) return kOrthographicError;
  *height = h;
  return kOrthographicHeight;
}

// the height `auto` stands for: the parallel view with the perspective view's extent at the plane through `at` (open-volume-renderer_amd/camera.py auto_height)
inline float auto_orthographic_height(const float from[3], const float at[3], float fovy_degrees)
{
  const double dx = (double)from[0] - at[0], dy = (double)from[1] - at[1], dz = (double)from[2] - at[2];
  return (float)(2.0 * std::sqrt(dx * dx + dy * dy + dz * dz) * std::tan((double)fovy_degrees * 0.5 * 3.14159265358979323846 / 180.0));
}

} // namespace ovrhip_plugin
