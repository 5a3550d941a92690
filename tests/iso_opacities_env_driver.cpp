// Driver of tests/test_isosurface_layers_env.py: plugin/isovalues_env.hpp's parse_iso_opacities on the CPU.  Exits 0 when every row of the table parsed to what
// the row expects.
#include "isovalues_env.hpp"

#include <cstdio>

int main()
{
  struct Row { const char* text; int count, n; float a[4]; };
  const Row t[] = {
    { "0.3,1", 2, 2, { 0.3f, 1.f } }, { "1", 1, 1, { 1.f } }, { "0.25,0.5,0.75,1", 4, 4, { 0.25f, 0.5f, 0.75f, 1.f } }, { "1e-3,5e-1", 2, 2, { 0.001f, 0.5f } },
    // refused: another count than the isovalues'
    { "0.3", 2, -1, {} }, { "0.3,1,0.5", 2, -1, {} }, { "0.3,1", 1, -1, {} }, { "0.1,0.2,0.3,0.4,0.5", 4, -1, {} },
    // refused: a value outside (0, 1]
    { "0,1", 2, -1, {} }, { "0.3,1.0001", 2, -1, {} }, { "-0.3,1", 2, -1, {} }, { "nan,1", 2, -1, {} }, { "0.3,inf", 2, -1, {} },
    // refused: never a shorter list than the user wrote - the whole string is parsed
    { "", 1, -1, {} }, { "0.3,abc", 2, -1, {} }, { "0.3,", 1, -1, {} }, { "0.3,", 2, -1, {} }, { ",0.3", 1, -1, {} }, { "0.3,,1", 2, -1, {} }, { "0.3x", 1, -1, {} }, { "0.3 1", 2, -1, {} },
    { "0.3;1", 2, -1, {} },
  };
  int failed = 0;
  for (const Row& r : t) {
    float a[5] = { 0, 0, 0, 0, 0 };
    const int n = ovrhip_plugin::parse_iso_opacities(r.text, a, r.count);
    bool ok = n == r.n;
    for (int k = 0; ok && k < r.n; ++k) ok = a[k] == r.a[k];
    if (!ok) { ++failed; printf("FAILED \"%s\" for %d isovalues: %d (%g, %g, %g, %g), expected %d\n", r.text, r.count, n, a[0], a[1], a[2], a[3], r.n); }
  }
  if (ovrhip_plugin::parse_iso_opacities(nullptr, nullptr, 2) != -1) { ++failed; printf("FAILED null\n"); }
  printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
