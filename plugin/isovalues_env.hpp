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

// OVR_HIP_ISO_OPACITIES beside OVR_HIP_ISOVALUES: "0.3,1" -> one opacity in (0, 1] per isovalue, parsed like the isovalues (the whole string).  `count`: the number
// of isovalues.  Returns count, or -1 for anything else: a list parse_isovalues refuses, another count than the isovalues', a value outside (0, 1] (a NaN included)
inline int parse_iso_opacities(const char* text, float* a, int count)
{
  const int n = parse_isovalues(text, a, count);
  if (n != count) return -1;
  for (int k = 0; k < n; ++k)
    if (!(a[k] > 0.f && a[k] <= 1.f)) return -1;
  return n;
}

} // namespace ovrhip_plugin
