// Driver of tests/test_ambient_occlusion_env.py: plugin/isovalues_env.hpp's parse_ao on the CPU.  Exits 0 when every row of the table parsed to what the row
// expects.
#include "isovalues_env.hpp"

#include <cmath>
#include <cstdio>

int main()
{
  struct Row { const char* samples; const char* distance; int rc, k; float r; };
  const float inf = INFINITY;
  const Row t[] = {
    { "8", nullptr, 0, 8, inf }, { "0", nullptr, 0, 0, inf }, { "16", "12", 0, 16, 12.f }, { "4", "2.5", 0, 4, 2.5f }, { "1", "inf", 0, 1, inf }, { "5", "1e-2", 0, 5, 0.01f },
    { "08", "3", 0, 8, 3.f },
    // refused: K
    { "", nullptr, -1, 0, 0 }, { "17", nullptr, -1, 0, 0 }, { "-1", nullptr, -1, 0, 0 }, { "+4", nullptr, -1, 0, 0 }, { "4.0", nullptr, -1, 0, 0 }, { "4 ", nullptr, -1, 0, 0 },
    { "8x", nullptr, -1, 0, 0 }, { "100", nullptr, -1, 0, 0 }, { "eight", nullptr, -1, 0, 0 },
    // refused: the radius
    { "8", "", -1, 0, 0 }, { "8", "0", -1, 0, 0 }, { "8", "-2", -1, 0, 0 }, { "8", "nan", -1, 0, 0 }, { "8", "3,4", -1, 0, 0 }, { "8", "3x", -1, 0, 0 }, { "8", "-inf", -1, 0, 0 },
  };
  int failed = 0;
  for (const Row& r : t) {
    int k = -7;
    float d = -7.f;
    const int rc = ovrhip_plugin::parse_ao(r.samples, r.distance, &k, &d);
    const bool ok = rc == r.rc && (rc != 0 ? (k == -7 && d == -7.f) : (k == r.k && d == r.r)); // (a refusal writes nothing)
    if (!ok) { ++failed; printf("FAILED \"%s\" / \"%s\": %d (%d, %g), expected %d (%d, %g)\n", r.samples, r.distance ? r.distance : "(unset)", rc, k, d, r.rc, r.k, r.r); }
  }
  int k = 0;
  float d = 0.f;
  if (ovrhip_plugin::parse_ao(nullptr, nullptr, &k, &d) != -1) { ++failed; printf("FAILED null\n"); }
  printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
