// Driver of tests/test_slices_env.py: the host arithmetic of ovr_hip_set_slices (csrc/host/slices_host.hpp) and the plugin's OVR_HIP_SLICES parser
// (plugin/slices_env.hpp) on the CPU, as literals.  A stand-alone program: the test builds it with -fsanitize=address,undefined and runs it.
#include "slices_env.hpp"
#include "slices_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } \
  } while (0)

using ovrhip::host::SliceValues;
using ovrhip::host::slice_values;
using ovrhip_plugin::SliceEnv;
using ovrhip_plugin::parse_slices;

static void host_values()
{
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  SliceValues v;
  { // an axis normal of any length: the unit axis, c the coordinate
    const float p[3] = { 3.f, -2.f, 5.5f }, n[3] = { 0.f, 0.f, 4.f };
    CHECK(slice_values(p, n, 0.f, 0, &v) == nullptr && v.normal[0] == 0.f && v.normal[1] == 0.f && v.normal[2] == 1.f && v.c == 5.5f, "axis: %g %g", (double)v.normal[2], (double)v.c);
  }
  { // (1, 2, -1) / sqrt(6) in float64, each component rounded; c from the ROUNDED normal in float64, rounded once
    const float p[3] = { 20.f, 16.5f, 9.f }, n[3] = { 1.f, 2.f, -1.f };
    CHECK(slice_values(p, n, 3.f, 3, &v) == nullptr, "oblique");
    const double l = std::sqrt(6.0);
    CHECK(v.normal[0] == (float)(1.0 / l) && v.normal[1] == (float)(2.0 / l) && v.normal[2] == (float)(-1.0 / l), "oblique normal");
    CHECK(v.c == (float)((double)v.normal[0] * 20.0 + (double)v.normal[1] * 16.5 + (double)v.normal[2] * 9.0), "oblique c %g", (double)v.c);
    CHECK(v.normal[0] == 0x1.a20bd8p-2f && v.normal[1] == 0x1.a20bd8p-1f && v.normal[2] == -0x1.a20bd8p-2f, "oblique normal, as literals: %a %a", (double)v.normal[0], (double)v.normal[1]);
  }
  { // a normal too short for float32 arithmetic is normalisable in float64; one too long as well
    const float p[3] = { 1.f, 1.f, 1.f }, tiny[3] = { 1e-30f, 0.f, 0.f }, huge[3] = { 3e38f, 3e38f, 0.f }, denorm[3] = { 0.f, 1e-45f, 0.f };
    CHECK(slice_values(p, tiny, inf, 2, &v) == nullptr && v.normal[0] == 1.f && v.c == 1.f, "tiny");
    CHECK(slice_values(p, huge, 0.f, 0, &v) == nullptr && v.normal[0] == (float)std::sqrt(0.5) && v.normal[1] == v.normal[0], "huge");
    CHECK(slice_values(p, denorm, 0.f, 0, &v) == nullptr && v.normal[1] == 1.f, "denormal");
  }
  const float p[3] = { 0.f, 0.f, 0.f }, n[3] = { 0.f, 1.f, 0.f };
  const float zero[3] = { 0.f, 0.f, 0.f }, nn[3] = { nan, 0.f, 1.f }, in[3] = { inf, 0.f, 0.f }, pn[3] = { 0.f, nan, 0.f }, pi[3] = { 0.f, 0.f, -inf };
  v.c = 42.f;
  CHECK(slice_values(p, zero, 0.f, 0, &v) != nullptr && slice_values(p, nn, 0.f, 0, &v) != nullptr && slice_values(p, in, 0.f, 0, &v) != nullptr, "normals that are refused");
  CHECK(slice_values(pn, n, 0.f, 0, &v) != nullptr && slice_values(pi, n, 0.f, 0, &v) != nullptr, "points that are refused");
  CHECK(slice_values(p, n, -1.f, 1, &v) != nullptr && slice_values(p, n, nan, 1, &v) != nullptr && slice_values(p, n, -0.f, 1, &v) == nullptr, "thicknesses");
  CHECK(slice_values(p, n, 2.f, 0, &v) != nullptr && slice_values(p, n, 2.f, 4, &v) != nullptr && slice_values(p, n, inf, -1, &v) != nullptr, "a slab's mode");
  CHECK(slice_values(p, n, 2.f, 1, &v) == nullptr && slice_values(p, n, 2.f, 3, &v) == nullptr && slice_values(p, n, 0.f, 17, &v) == nullptr, "a plane's mode is not read");
  CHECK(slice_values(p, n, 0.f, 0, nullptr) == nullptr, "validation alone");
  v.c = 42.f;
  (void)slice_values(p, zero, 0.f, 0, &v);
  CHECK(v.c == 42.f, "a refused slice writes nothing");
}

static bool same(const SliceEnv& s, float px, float py, float pz, float nx, float ny, float nz, float thickness, int mode)
{
  return s.point[0] == px && s.point[1] == py && s.point[2] == pz && s.normal[0] == nx && s.normal[1] == ny && s.normal[2] == nz && s.thickness == thickness && s.mode == mode;
}

static void env_parser()
{
  SliceEnv s[5];
  CHECK(parse_slices("1,2,3,0,0,1", s, 4) == 1 && same(s[0], 1, 2, 3, 0, 0, 1, 0, 1), "a plane");
  CHECK(parse_slices("1.5,-2,3e1,0.5,0,-1,4", s, 4) == 1 && same(s[0], 1.5f, -2, 30, 0.5f, 0, -1, 4, 1), "a slab, the default mode");
  CHECK(parse_slices("1,2,3,0,0,1,4,min", s, 4) == 1 && same(s[0], 1, 2, 3, 0, 0, 1, 4, 2), "a minimum slab");
  CHECK(parse_slices("1,2,3,0,0,1,inf,mean", s, 4) == 1 && std::isinf(s[0].thickness) && s[0].mode == 3, "the whole box");
  CHECK(parse_slices("1,2,3,0,0,1;4,5,6,1,0,0,2,max;7,8,9,0,1,0,0;0,0,0,1,1,1,1,mean", s, 4) == 4 && same(s[0], 1, 2, 3, 0, 0, 1, 0, 1) && same(s[1], 4, 5, 6, 1, 0, 0, 2, 1)
          && same(s[2], 7, 8, 9, 0, 1, 0, 0, 1) && same(s[3], 0, 0, 0, 1, 1, 1, 1, 3),
        "four slices, in the order given");
  const char* bad[] = { "", ";", "1,2,3,0,0", "1,2,3,0,0,1,", "1,2,3,0,0,1;", ";1,2,3,0,0,1", "1,2,3,0,0,1;;1,2,3,0,0,1", "1,2,3,0,0,1,4,median", "1,2,3,0,0,1,4,max,1", "1,2,3,0,0,1,4,maxi",
                        "1,2,3,0,0,1 ", " 1,2,3,0,0,1", "1,,3,0,0,1", "1,2,3,0,0,x", "1,2,3,0,0,1,max", "1,2,3,0,0,1,4,", "1,2,3,0,0,1,4,5",
                        "1,2,3,0,0,1;1,2,3,0,0,1;1,2,3,0,0,1;1,2,3,0,0,1;1,2,3,0,0,1", "1,2,3,0,0,1x" };
  for (const char* b : bad) CHECK(parse_slices(b, s, 4) == -1, "\"%s\" is refused", b);
  CHECK(parse_slices(nullptr, s, 4) == -1, "no string");
  CHECK(parse_slices("1,2,3,0,0,1;1,2,3,0,0,1", s, 1) == -1, "more than max");
  // a long string of digits: nothing is written past `max` entries, nothing read past the terminator
  std::string longs;
  for (int k = 0; k < 200; ++k) longs += "1,2,3,0,0,1;";
  CHECK(parse_slices(longs.c_str(), s, 4) == -1, "two hundred slices");
  // values the parser accepts and ovr_hip_set_slices refuses: parsing is not validation
  CHECK(parse_slices("1,2,3,0,0,0,-1", s, 4) == 1 && same(s[0], 1, 2, 3, 0, 0, 0, -1, 1), "a zero normal and a negative thickness parse");
  ovrhip::host::SliceValues v;
  CHECK(slice_values(s[0].point, s[0].normal, s[0].thickness, s[0].mode, &v) != nullptr, "and are refused by the setter's arithmetic");
}

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "host_values")) host_values();
  else if (argc == 2 && !strcmp(argv[1], "env_parser")) env_parser();
  else { printf("usage: driver host_values | env_parser\n"); return 2; }
  if (g_failed) printf("%d checks failed\n", g_failed);
  return g_failed ? 1 : 0;
}
