// slices_env.hpp - OVR_HIP_SLICES as data: "px,py,pz,nx,ny,nz[,thickness[,max|min|mean]];..." -> slices.  Pure (no HIP, no plugin state), so that
// tests/test_slices_env.py can hold it to a table on a machine without a GPU.
#pragma once

#include <cstdlib>
#include <cstring>

namespace ovrhip_plugin {

struct SliceEnv { float point[3], normal[3], thickness; int mode; }; // ovr_hip_slice's fields; mode: OVR_HIP_PROJECT_* (1 maximum - the default -, 2 minimum, 3 mean)

// one to `max` slices separated by single semicolons, each six to eight fields separated by single commas: the point, the normal, then optionally the thickness
// (a float, "inf" included; default 0: a plane) and the slab's mode (max, min or mean; default max).  The whole string is consumed: the number of slices, or -1
// for anything else (an empty string, slice or field, trailing text, a trailing separator, a ninth field, an unknown mode, more than `max` slices) - an error,
// never a shorter list than the user wrote.  Whether the VALUES make a slice (a zero normal, a negative thickness) is ovr_hip_set_slices' to say
inline int parse_slices(const char* text, SliceEnv* out, int max)
{
  if (!text || !*text) return -1;
  int n = 0;
  const char* c = text;
  for (;;) {
    if (n >= max) return -1;
    SliceEnv s{};
    s.mode = 1;
    float f[7] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    int fields = 0;
    for (;;) { // the numeric fields
      char* end = nullptr;
      if (*c == 0 || *c == ',' || *c == ';' || *c == ' ' || *c == '\t' || *c == '\n') return -1; // (strtof would skip white space)
      f[fields] = std::strtof(c, &end);
      if (end == c) return -1;
      ++fields;
      c = end;
      if (*c != ',') break;
      ++c;
      if (fields == 7) { // the eighth field: the mode's name
        static const char* const names[3] = { "max", "min", "mean" };
        int mode = 0;
        for (int k = 0; k < 3; ++k) {
          const size_t len = std::strlen(names[k]);
          if (std::strncmp(c, names[k], len) == 0 && (c[len] == 0 || c[len] == ';')) { mode = k + 1; c += len; }
        }
        if (mode == 0) return -1;
        s.mode = mode;
        ++fields;
        break;
      }
    }
    if (fields < 6) return -1;
    for (int a = 0; a < 3; ++a) { s.point[a] = f[a]; s.normal[a] = f[3 + a]; }
    s.thickness = f[6];
    out[n++] = s;
    if (*c == 0) return n;
    if (*c != ';' || c[1] == 0) return -1;
    ++c;
  }
}

} // namespace ovrhip_plugin
