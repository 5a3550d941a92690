// Driver of tests/test_gradient_opacity_host.py: csrc/host/gradient_opacity_host.hpp on the CPU - what the setter accepts and stores, the reciprocal, the
// activity rule, and OVR_HIP_GRADIENT_OPACITY as data.  `driver <scenario>` exits 0 when every row gave what it expects; `driver commit <mode> <lo> <hi>` prints
// the stored state's bit patterns (or "refused"), `driver parse <text>` the parsed thresholds', for the comparison with the numpy model.
#include "gradient_opacity_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace ovrhip;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } \
  } while (0)

static unsigned bits(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }

static void commit_rows()
{
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  GradientOpacityState s;
  CHECK(s.mode == 0 && s.lo == 0.f && s.hi == 1.f && s.inv_ramp == 1.f, "the default: OFF, (0, 1)");
  CHECK(gradient_opacity_commit(kGradientOpacityRamp, 0.f, 0.125f, &s) && s.mode == 1 && s.lo == 0.f && s.hi == 0.125f && s.inv_ramp == 8.f, "(0, 1/8): inv_ramp %g", s.inv_ramp);
  CHECK(gradient_opacity_commit(kGradientOpacityRamp, -1.f, 0.f, &s) && s.lo == -1.f && s.hi == 0.f && s.inv_ramp == 1.f, "the neutral ramp: lo may be negative");
  CHECK(gradient_opacity_commit(kGradientOpacityRamp, 0.02f, 0.06f, &s) && s.inv_ramp == 1.f / (0.06f - 0.02f), "1.f / (hi - lo) in float32");
  CHECK(gradient_opacity_commit(kGradientOpacityOff, 5.f, 2.f, &s) && s.mode == 0 && s.lo == 0.f && s.hi == 1.f && s.inv_ramp == 1.f, "OFF ignores the thresholds and stores (0, 1)");
  // refusals keep the state
  GradientOpacityState kept;
  gradient_opacity_commit(kGradientOpacityRamp, 0.25f, 0.5f, &kept);
  const GradientOpacityState before = kept;
  struct Row { int mode; float lo, hi; const char* what; };
  const Row rows[] = { { 2, 0.f, 1.f, "an unknown mode" }, { -1, 0.f, 1.f, "a negative mode" }, { 1, 1.f, 1.f, "lo == hi" }, { 1, 2.f, 1.f, "lo > hi" }, { 1, nan, 1.f, "NaN lo" },
                       { 1, 0.f, nan, "NaN hi" }, { 1, 0.f, inf, "infinite hi" }, { 1, -inf, 0.f, "infinite lo" }, { 0, nan, 1.f, "OFF with a NaN" }, { 0, 0.f, inf, "OFF with an infinity" },
                       { 1, -3e38f, 3e38f, "hi - lo overflows" } };
  for (const Row& r : rows) {
    CHECK(!gradient_opacity_commit(r.mode, r.lo, r.hi, &kept), "%s: refused", r.what);
    CHECK(!std::memcmp(&kept, &before, sizeof(kept)), "%s: the state stays", r.what);
  }
  CHECK(gradient_opacity_commit(kGradientOpacityRamp, 0.f, 1.f, nullptr) && !gradient_opacity_commit(3, 0.f, 1.f, nullptr), "a null out validates alone");
  // two neighbouring floats: the width is one ulp, the reciprocal finite
  const float a = 1.f, b = std::nextafter(1.f, 2.f);
  CHECK(gradient_opacity_commit(kGradientOpacityRamp, a, b, &s) && std::isfinite(s.inv_ramp) && s.inv_ramp == 8388608.f, "neighbours: inv_ramp %g", s.inv_ramp);
}

static void activity()
{
  for (int mode = 0; mode <= 2; ++mode)
    for (int march = 0; march <= 1; ++march)
      for (int shading = -1; shading <= 3; ++shading)
        for (int pre = 0; pre <= 1; ++pre) {
          const bool want = mode == 1 && march == 1 && (shading == 0 || shading == 1) && pre == 0;
          CHECK(gradient_opacity_active(mode, march != 0, shading, pre != 0) == want, "mode %d march %d shading %d pre %d", mode, march, shading, pre);
        }
  static_assert(gradient_opacity_active(1, true, 0, false) && gradient_opacity_active(1, true, 1, false) && !gradient_opacity_active(1, true, 2, false), "constexpr: NONE and GRADIENT, not FULL");
}

static void env_parser()
{
  float lo = -7.f, hi = -7.f;
  struct Good { const char* text; float lo, hi; };
  const Good good[] = { { "0,0.125", 0.f, 0.125f }, { "-1,0", -1.f, 0.f }, { "0.02,0.06", 0.02f, 0.06f }, { "1e-3,2.5e-1", 1e-3f, 0.25f }, { "+0.5,+2", 0.5f, 2.f }, { "-2,-1", -2.f, -1.f } };
  for (const Good& g : good) {
    CHECK(parse_gradient_opacity(g.text, &lo, &hi) && lo == g.lo && hi == g.hi, "\"%s\": %g %g", g.text, lo, hi);
    CHECK(parse_gradient_opacity(g.text, nullptr, nullptr), "\"%s\" with null outputs", g.text);
  }
  const char* bad[] = { "", ",", "1", "1,", ",1", "0,1,2", "0,1 ", "0,1x", "0;1", "a,b", "1,0", "1,1", "nan,1", "0,inf", "-inf,0", "0 ,1", "0,", "0,1,", "0.02-0.06", "-3e38,3e38" };
  for (const char* t : bad) {
    lo = hi = -7.f;
    CHECK(!parse_gradient_opacity(t, &lo, &hi) && lo == -7.f && hi == -7.f, "\"%s\": refused, the outputs untouched", t);
  }
  CHECK(!parse_gradient_opacity(nullptr, &lo, &hi), "a null pointer is not parsed");
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "commit", commit_rows }, { "activity", activity }, { "env_parser", env_parser } };

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const Scenario& s : kScenarios) printf("%s\n", s.name);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "state")) { // mode lo hi -> "mode lo hi inv_ramp" as hex bit patterns, or "refused"
    GradientOpacityState s;
    if (!gradient_opacity_commit(atoi(argv[2]), strtof(argv[3], nullptr), strtof(argv[4], nullptr), &s)) { printf("refused\n"); return 0; }
    printf("%d %08x %08x %08x\n", s.mode, bits(s.lo), bits(s.hi), bits(s.inv_ramp));
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "parse")) { // OVR_HIP_GRADIENT_OPACITY's value -> "lo hi" as hex bit patterns, or "refused"
    float lo = 0.f, hi = 0.f;
    if (!parse_gradient_opacity(argv[2], &lo, &hi)) { printf("refused\n"); return 0; }
    printf("%08x %08x\n", bits(lo), bits(hi));
    return 0;
  }
  for (const Scenario& s : kScenarios)
    if (argc == 2 && !strcmp(argv[1], s.name)) {
      s.run();
      if (g_failed) printf("%d checks failed\n", g_failed);
      return g_failed ? 1 : 0;
    }
  printf("usage: driver --list | <scenario> | state <mode> <lo> <hi> | parse <text>\n");
  return 2;
}
