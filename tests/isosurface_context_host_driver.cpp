// Driver of tests/test_isosurface_context_env.py: OVR_HIP_ISO_CONTEXT as the plugin parses it (plugin/iso_context_env.hpp), on the CPU, built with the address and
// undefined-behaviour sanitizers.  `driver <scenario>` exits 0 when every row of the scenario's table gave what the row expects.
#include "iso_context_env.hpp"

#include <cstdio>
#include <cstring>

using namespace ovrhip_plugin;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } \
  } while (0)

static void env_parser()
{
  struct Good { const char* text; float scale; };
  const Good good[] = { { "1", 1.f }, { "0", 0.f }, { "0.3", 0.3f }, { "1.0", 1.f }, { ".25", 0.25f }, { "5e-1", 0.5f }, { "-0", 0.f }, { "0x1p-2", 0.25f }, { "1e-40", 1e-40f } };
  for (const Good& g : good) {
    float s = -1.f;
    const bool ok = parse_iso_context(g.text, &s);
    CHECK(ok && s == g.scale && !std::signbit(s), "\"%s\": %d, %g", g.text, (int)ok, (double)s);
  }
  CHECK(parse_iso_context("0.5", nullptr), "a null output");
  const char* bad[] = { "", " ", " 0.5", "0.5 ", "0.5,", "0.5;1", "1.0001", "-0.1", "2", "nan", "inf", "-inf", "volume", "0.5f", "1e", "--1", "\t1", "1\n", "0,5" };
  for (const char* t : bad) {
    float s = -1.f;
    CHECK(!parse_iso_context(t, &s) && s == -1.f, "\"%s\" must be refused and leave the output alone (%g)", t, (double)s);
  }
  CHECK(!parse_iso_context(nullptr, nullptr), "a null pointer");
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "env_parser", env_parser } };

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const Scenario& s : kScenarios) printf("%s\n", s.name);
    return 0;
  }
  for (const Scenario& s : kScenarios)
    if (argc == 2 && !strcmp(argv[1], s.name)) {
      s.run();
      if (g_failed) printf("%d checks failed\n", g_failed);
      return g_failed ? 1 : 0;
    }
  printf("usage: driver --list | <scenario>\n");
  return 2;
}
