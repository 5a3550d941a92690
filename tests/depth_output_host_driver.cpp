// Driver of tests/test_depth_output_host.py: csrc/host/depth_output_host.hpp on the CPU - what the setter accepts, the activity rule, the resolved threshold
// depth, and OVR_HIP_DEPTH_OUTPUT_FILE (a raw little-endian float32 file) as data, held to max_depth_decode: what the encoder writes the depth limit's reader
// reads back bit for bit.  `driver <scenario>` exits 0 when every row gave what it expects; `driver check <mode> <threshold bits>` prints the rule that refused
// (0: accepted); `driver env <text>` parses OVR_HIP_DEPTH_OUTPUT; `driver read <path> <width> <height>` reads a file as OVR_HIP_MAX_DEPTH's reader does; `driver write <path> <width> <height> <layer bits ...>` writes the file of a layer (3 floats per pixel) and prints "written" or "refused".
#include "depth_output_host.hpp"

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
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), tiny = std::numeric_limits<float>::min();
  DepthOutputState s;
  CHECK(s.mode == kDepthOutputOff && s.threshold == 0.f, "the default: off");
  CHECK(depth_output_check(kDepthOutputOff, nan) == kDepthOutputOk && depth_output_check(kDepthOutputOff, -1.f) == kDepthOutputOk, "mode OFF does not read the threshold");
  CHECK(depth_output_check(kDepthOutputOn, 0.5f) == kDepthOutputOk && depth_output_check(kDepthOutputOn, tiny) == kDepthOutputOk && depth_output_check(kDepthOutputOn, 0.9999f) == kDepthOutputOk,
        "the smallest normal float, the median, the early-termination literal");
  CHECK(depth_output_check(kDepthOutputOn, std::nextafterf(0.f, 1.f)) == kDepthOutputOk, "any positive float, a denormal included");
  struct Row { int mode; float threshold; int rule; const char* what; };
  const Row rows[] = { { 2, 0.5f, kDepthOutputMode, "an unknown mode" }, { -1, 0.5f, kDepthOutputMode, "a negative mode" }, { 2, nan, kDepthOutputMode, "the mode is reported first" },
                       { 1, 0.f, kDepthOutputThreshold, "zero" }, { 1, -0.f, kDepthOutputThreshold, "minus zero" }, { 1, -0.5f, kDepthOutputThreshold, "negative" },
                       { 1, nan, kDepthOutputThreshold, "NaN" }, { 1, std::nextafterf(0.9999f, 1.f), kDepthOutputThreshold, "one float above 0.9999f" },
                       { 1, 1.f, kDepthOutputThreshold, "one" }, { 1, inf, kDepthOutputThreshold, "+inf" }, { 1, -inf, kDepthOutputThreshold, "-inf" } };
  for (const Row& r : rows) {
    CHECK(depth_output_check(r.mode, r.threshold) == r.rule, "%s: rule %d", r.what, depth_output_check(r.mode, r.threshold));
    CHECK(std::strlen(depth_output_rule_text(r.rule)) > 0, "%s: a message", r.what);
  }
  CHECK(std::strlen(depth_output_rule_text(kDepthOutputOk)) == 0, "no message without a refusal");
  float t = -1.f;
  CHECK(parse_depth_output("0.5", &t) && t == 0.5f && parse_depth_output("1e-38", nullptr) && parse_depth_output("0.9999", &t) && t == 0.9999f, "OVR_HIP_DEPTH_OUTPUT: a threshold");
  t = -1.f;
  CHECK(!parse_depth_output(nullptr, &t) && !parse_depth_output("", &t) && !parse_depth_output("0", &t) && !parse_depth_output("1", &t) && !parse_depth_output("nan", &t)
          && !parse_depth_output("0.5,", &t) && !parse_depth_output("0.5 ", &t) && !parse_depth_output("x", &t) && !parse_depth_output("-0.5", &t) && t == -1.f,
        "OVR_HIP_DEPTH_OUTPUT: refused, the output untouched");
}

static void activity()
{
  for (int on = 0; on <= 1; ++on)
    for (int march = 0; march <= 1; ++march)
      for (int shading = -1; shading <= 3; ++shading)
        for (int pre = 0; pre <= 1; ++pre)
          for (int gradop = 0; gradop <= 1; ++gradop) {
            const bool want = on == 1 && march == 1 && (shading == 0 || shading == 1) && pre == 0 && gradop == 0;
            CHECK(depth_output_active(on != 0, march != 0, shading, pre != 0, gradop != 0) == want, "on %d march %d shading %d pre %d gradop %d", on, march, shading, pre, gradop);
            // the depth limit's rule with a matching size is the same rule: a depth frame is drawn exactly where a depth-limited frame would be
            CHECK(max_depth_active(on != 0, march != 0, shading, pre != 0, gradop != 0, true) == want, "the depth limit's rule agrees");
            for (int md = 0; md <= 1; ++md)
              for (int same = 0; same <= 1; ++same)
                CHECK(depth_output_limited(want, md != 0, same != 0) == (want && md == 1 && same == 1), "limited: %d %d %d", (int)want, md, same);
          }
  static_assert(depth_output_active(true, true, 0, false, false) && depth_output_active(true, true, 1, false, false) && !depth_output_active(true, true, 2, false, false),
                "constexpr: NONE and GRADIENT, not FULL");
}

static void resolve()
{
  const float inf = std::numeric_limits<float>::infinity();
  CHECK(depth_output_threshold_depth(61.f, 1.f) == 61.f && depth_output_threshold_depth(20.f, 0.25f) == 80.f, "d_sum / share");
  CHECK(depth_output_threshold_depth(0.f, 0.f) == inf && depth_output_threshold_depth(5.f, 0.f) == inf && depth_output_threshold_depth(5.f, -1.f) == inf, "+inf where no sample reached");
  CHECK(bits(depth_output_threshold_depth(20.f, 1.f / 3.f)) == bits(20.f / (1.f / 3.f)), "one float32 division");
}

// encode, then decode with the depth limit's reader: equal bits, +inf, NaN payloads and denormals included
static void encoder()
{
  const unsigned patterns[] = { 0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0x7fc01234u, 0xffc00001u, 0x00000001u, 0x00800000u, 0x42742e14u, 0x7f7fffffu, 0x3f800000u };
  const int n = (int)(sizeof(patterns) / sizeof(patterns[0]));
  std::vector<float> values(n);
  for (int i = 0; i < n; ++i) std::memcpy(&values[i], &patterns[i], 4);
  std::vector<unsigned char> bytes;
  depth_output_encode(values.data(), (size_t)n, &bytes);
  CHECK(bytes.size() == (size_t)n * 4, "4 bytes per value");
  CHECK(bytes[4 * 9] == 0x14 && bytes[4 * 9 + 1] == 0x2e && bytes[4 * 9 + 2] == 0x74 && bytes[4 * 9 + 3] == 0x42, "little-endian: the low byte first");
  std::vector<float> back;
  CHECK(max_depth_decode(bytes.data(), bytes.size(), 4, 3, &back) && back.size() == (size_t)n, "the depth limit's reader takes it as a 4 x 3 image");
  for (int i = 0; i < n && i < (int)back.size(); ++i) {
    unsigned u;
    std::memcpy(&u, &back[i], 4);
    CHECK(u == patterns[i], "value %d: %08x came back as %08x", i, patterns[i], u);
  }
  CHECK(!max_depth_decode(bytes.data(), bytes.size(), 4, 4, nullptr) && !max_depth_decode(bytes.data(), bytes.size() - 1, 4, 3, nullptr), "any other size is refused");
  depth_output_encode(values.data(), 0, &bytes);
  CHECK(bytes.empty(), "no value, no byte");
  // the file: refusals in front of any write
  const float layer[6] = { 61.f, 31.f, 1.f, 0.f, 0.f, 0.f };
  CHECK(!depth_output_write_file(nullptr, layer, 2, 1) && !depth_output_write_file("", layer, 2, 1) && !depth_output_write_file("x", nullptr, 2, 1), "null arguments");
  CHECK(!depth_output_write_file("x", layer, 0, 1) && !depth_output_write_file("x", layer, 2, -1) && !depth_output_write_file("x", layer, 65536, 32768), "a size the depth limit refuses");
  CHECK(!depth_output_write_file("/nonexistent-directory/depth.f32", layer, 2, 1), "a path that cannot be opened");
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "check", check_rows }, { "activity", activity }, { "resolve", resolve }, { "encoder", encoder } };

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const Scenario& s : kScenarios) printf("%s\n", s.name);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "check")) {
    printf("%d\n", depth_output_check(std::atoi(argv[2]), from_bits((unsigned)std::strtoul(argv[3], nullptr, 16))));
    return 0;
  }
  if (argc >= 5 && !strcmp(argv[1], "write")) {
    const int w = std::atoi(argv[3]), h = std::atoi(argv[4]);
    std::vector<float> layer;
    for (int i = 5; i < argc; ++i) layer.push_back(from_bits((unsigned)std::strtoul(argv[i], nullptr, 16)));
    const bool fits = w > 0 && h > 0 && layer.size() == (size_t)w * (size_t)h * 3;
    printf("%s\n", fits && depth_output_write_file(argv[2], layer.data(), w, h) ? "written" : "refused");
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "env")) { // OVR_HIP_DEPTH_OUTPUT as the plugin parses it: the threshold's bits, or "refused"
    float t = 0.f;
    if (parse_depth_output(argv[2], &t)) printf("%08x\n", bits(t));
    else printf("refused\n");
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "read")) { // the file as OVR_HIP_MAX_DEPTH's reader takes it: the values' bits, or "refused"
    std::vector<float> depth;
    if (!max_depth_read_file(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), &depth)) { printf("refused\n"); return 0; }
    for (float v : depth) printf("%08x\n", bits(v));
    return 0;
  }
  for (const Scenario& s : kScenarios)
    if (argc == 2 && !strcmp(argv[1], s.name)) {
      s.run();
      if (g_failed) printf("%d checks failed\n", g_failed);
      return g_failed ? 1 : 0;
    }
  printf("usage: driver --list | <scenario> | check <mode> <threshold bits> | write <path> <width> <height> <layer bits ...>\n");
  return 2;
}
