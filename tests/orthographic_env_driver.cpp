// Driver of tests/test_camera_plan.py: plugin/orthographic_env.hpp on the CPU.  Exits 0 when every row of the table parsed to what the row expects.
#include "orthographic_env.hpp"

#include <cmath>
#include <cstdio>

int main()
{
  using namespace ovrhip_plugin;
  struct Row { const char* text; int kind; float height; };
  const Row t[] = {
    { "32", kOrthographicHeight, 32.f }, { "0.5", kOrthographicHeight, 0.5f }, { "1e3", kOrthographicHeight, 1000.f }, { "+16.25", kOrthographicHeight, 16.25f },
    { "auto", kOrthographicAuto, 0.f },
    // refused: never another camera than the user wrote
    { "", kOrthographicError, 0.f }, { "0", kOrthographicError, 0.f }, { "-4", kOrthographicError, 0.f }, { "inf", kOrthographicError, 0.f }, { "nan", kOrthographicError, 0.f },
    { "32x", kOrthographicError, 0.f }, { "32,16", kOrthographicError, 0.f }, { "32 ", kOrthographicError, 0.f }, { "Auto", kOrthographicError, 0.f }, { "auto ", kOrthographicError, 0.f },
    { "automatic", kOrthographicError, 0.f }, { "on", kOrthographicError, 0.f }, { "1e40", kOrthographicError, 0.f },
  };
  int failed = 0;
  for (const Row& r : t) {
    float h = 0.f;
    const int kind = parse_orthographic(r.text, &h);
    if (kind != r.kind || (kind == kOrthographicHeight && h != r.height) || (kind != kOrthographicHeight && h != 0.f)) {
      ++failed;
      printf("FAILED \"%s\": kind %d height %g, expected %d %g\n", r.text, kind, h, r.kind, r.height);
    }
  }
  float h = 0.f;
  if (parse_orthographic(nullptr, &h) != kOrthographicError) { ++failed; printf("FAILED null\n"); }
  // auto: 2 |from - at| tan(fovy / 2) - a 90 degree camera 16 away sees 32 at the plane through `at`
  const float from[3] = { 16.f, 8.f, 20.f }, at[3] = { 16.f, 8.f, 4.f };
  if (std::fabs(auto_orthographic_height(from, at, 90.f) - 32.f) > 1e-4f) { ++failed; printf("FAILED auto: %g\n", auto_orthographic_height(from, at, 90.f)); }
  printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
