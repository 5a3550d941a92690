// isovalues_env.hpp - OVR_HIP_ISOVALUES as data: "0.4,0.7" -> values.  Pure (no HIP, no plugin state), so that tests/test_isosurface_env.py can hold it to a
// table on a machine without a GPU.
#pragma once

#include <cmath>
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

// OVR_HIP_AO_SAMPLES and OVR_HIP_AO_DISTANCE beside OVR_HIP_ISOVALUES (ovr_hip_set_ambient_occlusion): K, an integer in 0 ... 16 written in decimal digits, and the
// radius in world units, a float > 0 or "inf" (unset: the whole box).  Each string is parsed whole.  Returns 0, or -1 for anything else: an empty string, a
// sign, trailing text, K above 16, a radius that is NaN or <= 0
inline int parse_ao(const char* samples, const char* distance, int* k, float* r)
{
  if (!samples || !*samples) return -1;
  int n = 0, digits = 0;
  for (const char* c = samples; *c; ++c, ++digits) {
    if (*c < '0' || *c > '9' || digits >= 2) return -1;
    n = 10 * n + (*c - '0');
  }
  if (n > 16) return -1;
  float d = INFINITY;
  if (distance) {
    float one[2];
    if (parse_isovalues(distance, one, 1) != 1 || !(one[0] > 0.f)) return -1;
    d = one[0];
  }
  *k = n; *r = d;
  return 0;
}

} // namespace ovrhip_plugin
