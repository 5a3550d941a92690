// Driver of tests/test_ambient_occlusion_plan.py: the ambient-occlusion part of csrc/host/launch_plan.hpp (LaunchFacts::ambient_occlusion,
// LaunchPlan::ambient_occlusion, isosurface_variant_exists) on the CPU.  `driver <scenario>` exits 0 when every row of the scenario gave what it expects.
#include "launch_plan.hpp"
#include "plan_compare.hpp"

#include <cstdio>
#include <cstring>

using namespace ovrhip;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } \
  } while (0)

// a 40 x 33 x 18 volume of the general layout under a 256 / 256 transfer function: mode 0
static LaunchFacts small(int elem = 4)
{
  LaunchFacts f;
  f.elem_bytes = elem; f.f32_general = elem == 4;
  f.nx = 40; f.ny = 33; f.nz = 18;
  f.stored_bytes = 1u << 20;
  f.n_color = f.n_alpha = 256;
  f.n_blocks_owned = f.n_schedule = 20;
  return f;
}
static LaunchOverrides ov(int addressing, int deep = -1) { LaunchOverrides o; o.addressing = addressing; o.deep = deep; return o; }

// every member of a plan but ambient_occlusion
static bool same_but_ao(LaunchPlan a, const LaunchPlan& b)
{
  a.ambient_occlusion = b.ambient_occlusion;
  return same_plan(a, b);
}

template <typename F> static int for_all_facts(F&& fn)
{
  int n = 0;
  for (int kind = 0; kind < 3; ++kind) // the march, a projection, isosurfaces
    for (int shading = 0; shading <= 2; ++shading)
      for (int bits = 0; bits < 2048; ++bits)
        for (int k = -1; k <= 3; k += 2) {
          LaunchFacts f = small(bits & 64 ? 2 : 4);
          f.shading = shading;
          f.pool = bits & 1; f.skipping = bits & 2; f.sparse = bits & 4; f.clip_on = bits & 8; f.lds_staging = bits & 16; f.reference_material = !(bits & 32);
          f.shadow_cache = bits & 128; f.ranges = bits & 2;
          if (bits & 256) { f.world = 4; f.n_blocks_owned = 10; }
          f.orthographic = bits & 512;
          f.translucent = bits & 1024;
          f.projection = kind == 1 ? 1 + (bits & 1) * 2 : 0; // maximum or mean
          f.isosurfaces = kind == 2 ? 1 + (bits & 3) : 0;
          fn(f, ov(k, bits & 256 ? 1 : -1), kind, shading, bits, k);
          ++n;
        }
  return n;
}

// ambient_occlusion == false: no plan has the flag, and the launcher's plans are what they were - literals of the launcher before the fact existed, and the fact
// is not read without isovalues or under OVR_HIP_SHADE_NONE
static void off_changes_nothing()
{
  LaunchFacts f = small();
  f.isosurfaces = 2; f.shading = 2; f.ranges = true;
  LaunchPlan p = plan_launch(f);
  CHECK(!p.error && p.isosurface.on && p.isosurface.skip && !p.isosurface.clipped && !p.isosurface.translucent && !p.ambient_occlusion && p.shading == 2 && p.am == 0
            && p.isosurface.lds_bytes == 384 && p.march_lds_bytes == 384 && !p.orthographic,
        "opaque, skipping: clipped %d lds %zu", (int)p.isosurface.clipped, p.isosurface.lds_bytes);
  f.translucent = true; f.shading = 1;
  p = plan_launch(f);
  CHECK(!p.error && p.isosurface.on && p.isosurface.skip && p.isosurface.clipped && p.isosurface.translucent && !p.ambient_occlusion && p.shading == 1, "translucent");
  f.translucent = false; f.clip_on = true; f.ranges = false; f.shading = 0;
  p = plan_launch(f);
  CHECK(!p.error && p.isosurface.on && !p.isosurface.skip && p.isosurface.clipped && !p.isosurface.translucent && !p.ambient_occlusion && p.shading == 0, "opaque, clipped");
  const int n = for_all_facts([](LaunchFacts f, const LaunchOverrides& o, int kind, int shading, int bits, int k) {
    const LaunchPlan a = plan_launch(f, o);
    CHECK(!a.ambient_occlusion, "kind %d shading %d bits %d override %d: the flag without the fact", kind, shading, bits, k);
    CHECK(a.error || plan_variants_exist(a, f.f32_general), "kind %d shading %d bits %d override %d: the plan names a variant that does not exist", kind, shading, bits, k);
    if (!a.error && kind == 2)
      CHECK(a.isosurface.clipped == (f.clip_on || f.orthographic || f.translucent) && a.isosurface.skip == f.ranges && a.isosurface.translucent == f.translucent,
            "isosurface bits %d: clipped %d skip %d translucent %d", bits, (int)a.isosurface.clipped, (int)a.isosurface.skip, (int)a.isosurface.translucent);
    if (kind != 2 || shading == 0) { // the fact is a shaded isosurface frame's alone
      LaunchFacts g = f;
      g.ambient_occlusion = true;
      const LaunchPlan b = plan_launch(g, o);
      CHECK(same_but_ao(a, b) && !b.ambient_occlusion, "kind %d shading %d bits %d override %d: the fact changed a plan without an ambient term on a surface", kind, shading, bits, k);
    }
  });
  CHECK(n == 3 * 3 * 2048 * 3, "%d plans", n);
}

// an AO plan IS the translucent clipped plan of the same frame plus one flag, under GRADIENT and FULL; the error cases are that frame's
static void sweep()
{
  int seen = 0;
  for_all_facts([&](LaunchFacts f, const LaunchOverrides& o, int kind, int shading, int bits, int k) {
    if (kind != 2 || shading == 0) return;
    LaunchFacts g = f;
    g.ambient_occlusion = true;
    const LaunchPlan p = plan_launch(g, o);
    LaunchFacts c = f;
    c.translucent = true; c.clip_on = true;
    const LaunchPlan q = plan_launch(c, o);
    if (p.error || q.error) { CHECK(p.error == q.error, "shading %d bits %d: error %d vs %d", shading, bits, (int)p.error, (int)q.error); return; }
    CHECK(p.ambient_occlusion && !q.ambient_occlusion && p.isosurface.translucent && p.isosurface.clipped && p.isosurface.skip == f.ranges && p.shading == shading,
          "shading %d bits %d override %d: ao %d translucent %d clipped %d", shading, bits, k, (int)p.ambient_occlusion, (int)p.isosurface.translucent, (int)p.isosurface.clipped);
    CHECK(same_but_ao(p, q), "shading %d bits %d override %d: not the translucent clipped frame's plan", shading, bits, k);
    CHECK(plan_variants_exist(p, g.f32_general) && isosurface_variant_exists(p.shading, p.am, p.isosurface.skip, p.isosurface.clipped, p.orthographic, true, true),
          "shading %d bits %d override %d: the plan names a variant that does not exist", shading, bits, k);
    ++seen;
  });
  CHECK(seen == 2 * 2048 * 3, "%d AO plans", seen);
  LaunchFacts f = small();
  f.ambient_occlusion = true; f.shading = 2; f.isosurfaces = 5;
  CHECK(plan_launch(f).error, "five isovalues");
  f.isosurfaces = 2; f.quad = true;
  CHECK(plan_launch(f).error, "a quad replica");
}

// the predicate the kernels' static_asserts ask
static void variants()
{
  int n = 0;
  for (int shade = -1; shade <= 3; ++shade)
    for (int am = -1; am <= 5; ++am)
      for (int bits = 0; bits < 16; ++bits) {
        const bool skip = bits & 1, clipped = bits & 2, ortho = bits & 4, trans = bits & 8;
        const bool want = shade >= 1 && shade <= 2 && am >= 0 && am <= 4 && clipped && trans;
        CHECK(isosurface_variant_exists(shade, am, skip, clipped, ortho, trans, true) == want, "shade %d am %d bits %d", shade, am, bits);
        CHECK(isosurface_variant_exists(shade, am, skip, clipped, ortho, trans, false) == isosurface_variant_exists(shade, am, skip, clipped, ortho, trans), "the default is false");
        n += want;
      }
  CHECK(n == 2 * 5 * 2 * 2, "%d AO variants per type: shading x addressing x skip x camera", n);
  static_assert(isosurface_variant_exists(2, 4, true, true, true, true, true) && !isosurface_variant_exists(0, 4, true, true, false, true, true), "usable in a static_assert");
}

int main(int argc, char** argv)
{
  struct S { const char* name; void (*run)(); };
  const S all[] = { { "off_changes_nothing", off_changes_nothing }, { "sweep", sweep }, { "variants", variants } };
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const S& s : all) printf("%s\n", s.name);
    return 0;
  }
  for (const S& s : all)
    if (argc == 2 && !strcmp(argv[1], s.name)) {
      s.run();
      printf("%s: %d failed\n", s.name, g_failed);
      return g_failed ? 1 : 0;
    }
  printf("usage: driver --list | <scenario>\n");
  return 2;
}
