// Driver of tests/test_isosurface_env.py: plugin/isovalues_env.hpp on the CPU.  Exits 0 when every row of the table parsed to what the row expects.
#include "isovalues_env.hpp"

#include <cstdio>
#include <cstring>

int main()
{
  struct Row { const char* text; int n; float v[4]; };
  const Row t[] = {
    { "0.4", 1, { 0.4f } }, { "0.7,0.4", 2, { 0.7f, 0.4f } }, { "1,2,3,4", 4, { 1.f, 2.f, 3.f, 4.f } }, { "-1.5e2,+3", 2, { -150.f, 3.f } }, { "300", 1, { 300.f } },
    // refused: never a shorter list than the user wrote
    { "", -1, {} }, { "0.4,abc", -1, {} }, { "0.4,", -1, {} }, { ",0.4", -1, {} }, { "0.4,,0.7", -1, {} }, { "0.4x", -1, {} }, { "0.4 0.7", -1, {} }, { "1,2,3,4,5", -1, {} },
    { "abc", -1, {} }, { "0.4;0.7", -1, {} },
  };
  int failed = 0;
  for (const Row& r : t) {
    float v[5] = { 0, 0, 0, 0, 0 };
    const int n = ovrhip_plugin::parse_isovalues(r.text, v, 4);
    bool ok = n == r.n;
    for (int k = 0; ok && k < r.n; ++k) ok = v[k] == r.v[k];
    if (!ok) { ++failed; printf("FAILED \"%s\": %d values (%g, %g, %g, %g), expected %d\n", r.text, n, v[0], v[1], v[2], v[3], r.n); }
  }
  if (ovrhip_plugin::parse_isovalues(nullptr, nullptr, 4) != -1) { ++failed; printf("FAILED null\n"); }
  printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
