// Driver of tests/test_preintegration_host.py: the host side of pre-integrated classification (csrc/host/preintegration_host.hpp) on the CPU - the node table,
// the subdivision the LDS budget allows and OVR_HIP_PREINTEGRATION as data.  Plain C++, no ROCm headers; the test builds it a second time with the address and
// undefined-behaviour sanitizers.  `driver <scenario>` exits 0 when every row of the scenario's table gave what the row expects; `driver nodes <file>` reads
// (n_color, n_alpha, subdivision as int32, then n_color rgba quadruples and n_alpha alphas as float32) and prints M and the 4 * (M + 1) floats of the table as
// bit patterns, which the test holds to the numpy model's.
#include "preintegration_host.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace ovrhip;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } \
  } while (0)

static int nodes(const char* path)
{
  FILE* f = fopen(path, "rb");
  if (!f) { printf("cannot open %s\n", path); return 2; }
  int32_t head[3] = { 0, 0, 0 };
  if (fread(head, sizeof(int32_t), 3, f) != 3 || head[0] < 1 || head[1] < 1 || head[0] > (1 << 20) || head[1] > (1 << 20)) { fclose(f); printf("bad header\n"); return 2; }
  std::vector<float> colors((size_t)head[0] * 4), alphas((size_t)head[1]);
  const bool ok = fread(colors.data(), sizeof(float), colors.size(), f) == colors.size() && fread(alphas.data(), sizeof(float), alphas.size(), f) == alphas.size();
  fclose(f);
  if (!ok) { printf("short file\n"); return 2; }
  std::vector<float> out;
  const int m = build_preintegration_nodes(colors.data(), head[0], alphas.data(), head[1], head[2], out);
  printf("%d\n", m);
  if (m > 0) {
    if (out.size() != (size_t)4 * ((size_t)m + 1)) { printf("size %zu\n", out.size()); return 1; }
    for (float v : out) {
      uint32_t b;
      memcpy(&b, &v, 4);
      printf("%08x\n", b);
    }
  }
  return 0;
}

// M, the table's bytes, S by the room, and the refusal
static void subdivision()
{
  CHECK(preintegration_segments(256, 256) == 255 && preintegration_segments(16, 64) == 63 && preintegration_segments(64, 16) == 63 && preintegration_segments(1, 1) == 1
          && preintegration_segments(2, 1) == 1 && preintegration_segments(1, 3) == 2, "max(n_alpha - 1, n_color - 1, 1)");
  CHECK(preintegration_nodes(256, 256, 4) == 1021 && preintegration_nodes(256, 256, 2) == 511 && preintegration_nodes(256, 256, 1) == 256 && preintegration_nodes(1, 1, 4) == 5
          && preintegration_nodes(16, 64, 4) == 253, "M = S * segments + 1");
  CHECK(preintegration_table_bytes(1021) == 16352 && preintegration_table_bytes(1) == 32, "16 * (M + 1)");
  struct Row { int nc, na; size_t room; int s; };
  const Row rows[] = {
    { 256, 256, 16352, 4 }, { 256, 256, 16351, 2 }, { 256, 256, 8192, 2 }, { 256, 256, 8191, 1 }, { 256, 256, 4112, 1 }, { 256, 256, 4111, 0 }, { 256, 256, 0, 0 },
    { 1, 1, 96, 4 }, { 1, 1, 95, 2 }, { 1, 1, 64, 2 }, { 1, 1, 63, 1 }, { 1, 1, 48, 1 }, { 1, 1, 47, 0 },
    { 16, 64, 1u << 20, 4 }, { 4096, 16, 49152, 0 }, { 4096, 16, 65552, 1 }, { 4096, 16, 131088, 2 },
  };
  for (const Row& r : rows) CHECK(preintegration_subdivision(r.nc, r.na, r.room) == r.s, "n_color %d n_alpha %d room %zu: %d, expected %d", r.nc, r.na, r.room, preintegration_subdivision(r.nc, r.na, r.room), r.s);
  // the builder's refusals leave the output alone
  std::vector<float> out(3, 7.f);
  const float c[4] = { 1.f, 0.5f, 0.25f, 1.f }, a[1] = { 0.5f };
  CHECK(build_preintegration_nodes(nullptr, 1, a, 1, 4, out) == 0 && build_preintegration_nodes(c, 1, nullptr, 1, 4, out) == 0 && build_preintegration_nodes(c, 0, a, 1, 4, out) == 0
          && build_preintegration_nodes(c, 1, a, 0, 4, out) == 0 && build_preintegration_nodes(c, 1, a, 1, 0, out) == 0 && out.size() == 3 && out[0] == 7.f, "refusals");
  // a one-entry pair: five nodes of a constant tau = 1 (a = 0.5) - T = u, K = u * c, and the copy of the last
  CHECK(build_preintegration_nodes(c, 1, a, 1, 4, out) == 5 && out.size() == 24, "one entry each: %zu floats", out.size());
  for (int j = 0; j < 5 && out.size() == 24; ++j)
    CHECK(out[4 * j] == 0.25f * j && out[4 * j + 1] == 0.25f * j && out[4 * j + 2] == 0.125f * j && out[4 * j + 3] == 0.0625f * j, "node %d: %g %g %g %g", j, out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
  if (out.size() == 24) CHECK(!memcmp(&out[20], &out[16], 16), "the copy of the last node");
  // an opaque entry: tau is capped at 24, never infinite
  const float one[2] = { 1.f, 2.f };
  const float c2[8] = { 0, 0, 0, 1, 1, 1, 1, 1 };
  CHECK(build_preintegration_nodes(c2, 2, one, 2, 1, out) == 2 && out[4] == 24.f && out[5] == 12.f, "a = 1 (and a > 1, clamped): T %g K %g", out[4], out[5]);
}

static void env_parser()
{
  int m = -1;
  CHECK(parse_preintegration("0", &m) && m == 0, "\"0\": %d", m);
  CHECK(parse_preintegration("1", &m) && m == 1, "\"1\": %d", m);
  CHECK(parse_preintegration("1", nullptr), "a null output");
  const char* bad[] = { "", " ", " 1", "1 ", "2", "-1", "01", "10", "1.0", "on", "segments", "+1", "\t1", "1\n", "0x1" };
  for (const char* t : bad) {
    m = -1;
    CHECK(!parse_preintegration(t, &m) && m == -1, "\"%s\" must be refused and leave the output alone (%d)", t, m);
  }
  CHECK(!parse_preintegration(nullptr, nullptr), "a null pointer");
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "subdivision", subdivision }, { "env_parser", env_parser } };

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const Scenario& s : kScenarios) printf("%s\n", s.name);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "nodes")) return nodes(argv[2]);
  for (const Scenario& s : kScenarios)
    if (argc == 2 && !strcmp(argv[1], s.name)) {
      s.run();
      if (g_failed) printf("%d checks failed\n", g_failed);
      return g_failed ? 1 : 0;
    }
  printf("usage: driver --list | <scenario> | nodes <file>\n");
  return 2;
}
