// Driver of tests/test_max_depth_host.py: csrc/host/max_depth_host.hpp on the CPU - what the setter accepts, the activity rule, the cut, and OVR_HIP_MAX_DEPTH
// (a raw little-endian float32 file) as data.  `driver <scenario>` exits 0 when every row gave what it expects; `driver check <mem_kind> <width> <height>`
// prints the rule that refused (0: accepted), `driver cut <t1 bits> <z bits>` the cut's bit pattern, `driver file <path> <width> <height>` the values' bit
// patterns (or "refused"), for the comparison with the numpy model.
#include "max_depth_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

using namespace ovrhip;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } \
  } while (0)

static unsigned bits(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }
static float from_bits(unsigned u) { float x; std::memcpy(&x, &u, 4); return x; }

static void check_rows()
{
  const float image[4] = { 0.f, 1.f, 2.f, 3.f };
  MaxDepthState s;
  CHECK(!s.on && s.width == 0 && s.height == 0, "the default: off");
  CHECK(max_depth_check(image, 0, 2, 2) == kMaxDepthOk && max_depth_check(image, 1, 4, 1) == kMaxDepthOk, "host and device memory");
  CHECK(max_depth_check(nullptr, 7, -3, 0) == kMaxDepthOk, "a null image switches the limit off: the other arguments are not read");
  struct Row { int mem_kind; long long w, h; int rule; const char* what; };
  const Row rows[] = { { 2, 2, 2, kMaxDepthMemKind, "an unknown mem_kind" }, { -1, 2, 2, kMaxDepthMemKind, "a negative mem_kind" }, { 0, 0, 2, kMaxDepthExtent, "width 0" },
                       { 0, 2, 0, kMaxDepthExtent, "height 0" }, { 1, -4, 2, kMaxDepthExtent, "a negative width" }, { 0, 2, -1, kMaxDepthExtent, "a negative height" },
                       { 0, 65536, 32768, kMaxDepthOverflow, "2^31 pixels" }, { 0, 2147483647, 2, kMaxDepthOverflow, "the product overflows 32 bits" },
                       { 0, 2147483647, 2147483647, kMaxDepthOverflow, "the product overflows 62 bits" }, { 0, 4294967296ll, 1, kMaxDepthOverflow, "a width beyond 32 bits" },
                       { 2, 0, 0, kMaxDepthMemKind, "mem_kind is reported first" } };
  for (const Row& r : rows) {
    CHECK(max_depth_check(image, r.mem_kind, r.w, r.h) == r.rule, "%s: rule %d", r.what, max_depth_check(image, r.mem_kind, r.w, r.h));
    CHECK(std::strlen(max_depth_rule_text(r.rule)) > 0, "%s: a message", r.what);
  }
  CHECK(max_depth_check(image, 0, 2147483647, 1) == kMaxDepthOk && max_depth_check(image, 0, 46340, 46340) == kMaxDepthOk && max_depth_check(image, 0, 46341, 46341) == kMaxDepthOverflow,
        "2^31 - 1 pixels are the most");
  CHECK(std::strlen(max_depth_rule_text(kMaxDepthOk)) == 0, "no message without a refusal");
}

static void activity()
{
  for (int on = 0; on <= 1; ++on)
    for (int march = 0; march <= 1; ++march)
      for (int shading = -1; shading <= 3; ++shading)
        for (int pre = 0; pre <= 1; ++pre)
          for (int gradop = 0; gradop <= 1; ++gradop)
            for (int same = 0; same <= 1; ++same) {
              const bool want = on == 1 && march == 1 && (shading == 0 || shading == 1) && pre == 0 && gradop == 0 && same == 1;
              CHECK(max_depth_active(on != 0, march != 0, shading, pre != 0, gradop != 0, same != 0) == want, "on %d march %d shading %d pre %d gradop %d same %d", on, march, shading, pre, gradop, same);
            }
  static_assert(max_depth_active(true, true, 0, false, false, true) && max_depth_active(true, true, 1, false, false, true) && !max_depth_active(true, true, 2, false, false, true),
                "constexpr: NONE and GRADIENT, not FULL");
  MaxDepthState s;
  s.on = true; s.width = 37; s.height = 23;
  CHECK(max_depth_size_matches(s, 37, 23) && !max_depth_size_matches(s, 23, 37) && !max_depth_size_matches(s, 37, 24) && !max_depth_size_matches(s, 0, 0), "the image's size is the framebuffer's");
}

static void cut()
{
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  CHECK(max_depth_cut(5.f, inf) == 5.f && max_depth_cut(5.f, nan) == 5.f, "+inf and NaN: no surface");
  CHECK(max_depth_cut(5.f, 7.f) == 5.f && max_depth_cut(5.f, 5.f) == 5.f && max_depth_cut(5.f, 3.f) == 3.f, "fmin(t1, z)");
  CHECK(max_depth_cut(5.f, -2.f) == -2.f && max_depth_cut(5.f, -inf) == -inf && max_depth_cut(5.f, 0.f) == 0.f, "in front of the ray's origin");
  CHECK(max_depth_cut(3.4028235e38f, 1e38f) == 1e38f, "the box test's FLT_MAX");
}

// the file's bytes: exactly width * height little-endian floats
static void file_parser()
{
  const float inf = std::numeric_limits<float>::infinity();
  const float want[6] = { 0.f, 1.5f, -2.25f, inf, 61.32f, 1e-30f };
  unsigned char bytes[25];
  for (int i = 0; i < 6; ++i) {
    const unsigned u = bits(want[i]);
    for (int b = 0; b < 4; ++b) bytes[4 * i + b] = (unsigned char)(u >> (8 * b));
  }
  bytes[24] = 0;
  std::vector<float> out(3, -7.f);
  CHECK(max_depth_decode(bytes, 24, 3, 2, &out) && out.size() == 6, "3 x 2");
  for (int i = 0; i < 6 && i < (int)out.size(); ++i) CHECK(bits(out[i]) == bits(want[i]), "value %d: %08x", i, bits(out[i]));
  CHECK(max_depth_decode(bytes, 24, 6, 1, &out) && max_depth_decode(bytes, 24, 1, 6, nullptr), "the same bytes as 6 x 1 and 1 x 6; a null output validates alone");
  const unsigned nan_bits = 0x7fc01234u;
  unsigned char nb[4] = { 0x34, 0x12, 0xc0, 0x7f };
  CHECK(max_depth_decode(nb, 4, 1, 1, &out) && out.size() == 1 && bits(out[0]) == nan_bits, "a NaN keeps its payload");
  out.assign(2, -7.f);
  struct Bad { size_t n; int w, h; const char* what; };
  const Bad bad[] = { { 23, 3, 2, "a byte short" }, { 25, 3, 2, "a byte long" }, { 24, 3, 3, "too few values" }, { 24, 2, 2, "too many values" }, { 0, 3, 2, "an empty file" },
                      { 24, 0, 6, "width 0" }, { 24, 6, 0, "height 0" }, { 24, -3, -2, "negative extents" } };
  for (const Bad& b : bad) CHECK(!max_depth_decode(bytes, b.n, b.w, b.h, &out) && out.size() == 2 && out[0] == -7.f, "%s: refused, the output untouched", b.what);
  CHECK(!max_depth_decode(nullptr, 24, 3, 2, &out), "a null pointer");
  CHECK(!max_depth_read_file(nullptr, 3, 2, &out) && !max_depth_read_file("", 3, 2, &out) && !max_depth_read_file("/nonexistent/depth.f32", 3, 2, &out) && out.size() == 2, "no file");
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "check", check_rows }, { "activity", activity }, { "cut", cut }, { "file_parser", file_parser } };

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const Scenario& s : kScenarios) printf("%s\n", s.name);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "check")) { // mem_kind width height -> the rule (0: accepted)
    const float x = 0.f;
    printf("%d\n", max_depth_check(&x, atoi(argv[2]), atoll(argv[3]), atoll(argv[4])));
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "cut")) { // t1 and z as hex bit patterns -> the cut's
    printf("%08x\n", bits(max_depth_cut(from_bits((unsigned)strtoul(argv[2], nullptr, 16)), from_bits((unsigned)strtoul(argv[3], nullptr, 16)))));
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "file")) { // path width height -> the values as hex bit patterns, or "refused"
    std::vector<float> v;
    if (!max_depth_read_file(argv[2], atoi(argv[3]), atoi(argv[4]), &v)) { printf("refused\n"); return 0; }
    for (float f : v) printf("%08x ", bits(f));
    printf("\n");
    return 0;
  }
  for (const Scenario& s : kScenarios)
    if (argc == 2 && !strcmp(argv[1], s.name)) {
      s.run();
      if (g_failed) printf("%d checks failed\n", g_failed);
      return g_failed ? 1 : 0;
    }
  printf("usage: driver --list | <scenario> | check <mem_kind> <width> <height> | cut <t1 bits> <z bits> | file <path> <width> <height>\n");
  return 2;
}
