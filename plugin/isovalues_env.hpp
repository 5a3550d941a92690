// isovalues_env.hpp - OVR_HIP_ISOVALUES as data: "0.4,0.7" -> values.  Pure (no HIP, no plugin state), so that tests/test_isosurface_env.py can hold it to a
// table on a machine without a GPU.
#pragma once

#include <cstdio>

namespace ovrhip_plugin {

// one to `max` floats separated by single commas, the whole string consumed: the number of values, or -1 for anything else (an empty string or field, trailing
// text, a trailing comma, more than `max` values) - an error, never a shorter list than the user wrote
inline int parse_isovalues(const char* text, float* v, int max)
{
  if (!text || !*text) return -1;
  int n = 0;
  for (const char* c = text; *c;) {
    int used = 0;
    if (n >= max || std::sscanf(c, "%f%n", &v[n], &used) != 1 || used <= 0) return -1;
    if (c[used] != 0 && !(c[used] == ',' && c[used + 1] != 0)) return -1;
    ++n;
    c += used + (c[used] == ',' ? 1 : 0);
  }
  return n;
}

} // namespace ovrhip_plugin
