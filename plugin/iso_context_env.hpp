// iso_context_env.hpp - OVR_HIP_ISO_CONTEXT as data: "<scale in [0, 1]>" -> the opacity scale of the volume marched around the level sets
// (ovr_hip_set_isosurface_context in mode VOLUME).  Pure (no HIP, no plugin state), so that tests/test_isosurface_context_env.py can hold it to a table on a
// machine without a GPU.
#pragma once

#include <cmath>
#include <cstdlib>

namespace ovrhip_plugin {

// one float, the whole string: true and *scale set, or false for anything else - an empty string, leading white space, trailing text, a NaN, a value below 0
// or above 1 ("inf" included) - an error, never a default the user did not write.  -0 is 0.  Unset (a null pointer) is not parsed: the plugin calls nothing
inline bool parse_iso_context(const char* text, float* scale)
{
  if (!text || !*text || *text == ' ' || *text == '\t' || *text == '\n') return false; // (strtof would skip white space)
  char* end = nullptr;
  const float v = std::strtof(text, &end);
  if (end == text || *end != 0) return false;
  if (!(v >= 0.f && v <= 1.f)) return false; // (a NaN fails both comparisons)
  if (scale) *scale = v == 0.f ? 0.f : v;
  return true;
}

} // namespace ovrhip_plugin
