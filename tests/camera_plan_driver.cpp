// Driver of tests/test_camera_plan.py: the orthographic part of csrc/host/launch_plan.hpp on the CPU.  `driver <scenario>` exits 0 when every row of the
// scenario's table gave what the row expects.
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

// a 40 x 33 x 18 volume under a 256 / 256 transfer function: mode 0
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

// the same plan but for the camera flag
static bool same_but_orthographic(LaunchPlan a, const LaunchPlan& b)
{
  a.orthographic = b.orthographic;
  return same_plan(a, b);
}

template <typename F> static int for_all_facts(F&& fn)
{
  int n = 0;
  for (int kind = 0; kind < 3; ++kind) // the march, a projection, isosurfaces
    for (int shading = 0; shading <= 2; ++shading)
      for (int bits = 0; bits < 512; ++bits)
        for (int k = -1; k <= 3; k += 2) {
          LaunchFacts f = small(bits & 64 ? 2 : 4);
          f.shading = shading;
          f.pool = bits & 1; f.skipping = bits & 2; f.sparse = bits & 4; f.clip_on = bits & 8; f.lds_staging = bits & 16; f.reference_material = !(bits & 32);
          f.shadow_cache = bits & 128; f.ranges = bits & 2;
          if (bits & 256) { f.world = 4; f.n_blocks_owned = 10; }
          f.projection = kind == 1 ? 1 + (bits & 1) * 2 : 0; // maximum or mean
          f.isosurfaces = kind == 2 ? 2 : 0;
          fn(f, ov(k, bits & 256 ? 1 : -1), kind, shading, bits, k);
          ++n;
        }
  return n;
}

// orthographic == false: the field changes no plan, and no plan without it is orthographic
static void off_changes_nothing()
{
  // plans of the parent as literals: the unshaded LDS-staged march, the deep pooled march of a small shard, a clipped shaded in-place march
  LaunchFacts f = small();
  f.lds_staging = true;
  LaunchPlan p = plan_launch(f);
  CHECK(!p.error && p.march.lds_staged && !p.march.clipped && !p.orthographic && p.lds_brick_offset == 5536, "LDS-staged: offset %u", p.lds_brick_offset);
  f = small(); f.shading = 2; f.pool = true; f.world = 4; f.n_blocks_owned = 10;
  p = plan_launch(f);
  CHECK(!p.error && p.pooled && p.march.deep && !p.shade.material && !p.shade.clipped && !p.orthographic, "deep: %d", (int)p.march.deep);
  f = small(); f.shading = 1; f.clip_on = true;
  p = plan_launch(f);
  CHECK(!p.error && !p.pooled && p.march.clipped && p.march.material && !p.orthographic, "clipped in place");
  const int n = for_all_facts([](LaunchFacts f, const LaunchOverrides& o, int kind, int shading, int bits, int k) {
    const LaunchPlan a = plan_launch(f, o);
    CHECK(!a.orthographic, "kind %d shading %d bits %d override %d: orthographic without the fact", kind, shading, bits, k);
    CHECK(a.error || plan_variants_exist(a, f.f32_general), "kind %d shading %d bits %d override %d: the plan names a variant that does not exist", kind, shading, bits, k);
    // what the clip box alone decides is what it decided: the clipped flags follow clip_on
    if (!a.error && kind == 0 && !a.march.lds_staged) CHECK(a.march.clipped == f.clip_on, "kind 0 shading %d bits %d: clipped %d", shading, bits, (int)a.march.clipped);
    if (!a.error && kind == 1) CHECK(a.project.clipped == f.clip_on, "projection: clipped");
    if (!a.error && kind == 2) CHECK(a.isosurface.clipped == f.clip_on, "isosurface: clipped");
  });
  CHECK(n == 3 * 3 * 512 * 3, "%d plans", n);
}

// an orthographic frame plans the clipped variants - exactly the plan of the same frame with a clip box -, never LDS staging, never deep rounds
static void orthographic_plans()
{
  for_all_facts([](LaunchFacts f, const LaunchOverrides& o, int kind, int shading, int bits, int k) {
    LaunchFacts g = f;
    g.orthographic = true;
    const LaunchPlan p = plan_launch(g, o);
    LaunchFacts c = f;
    c.clip_on = true;
    LaunchPlan q = plan_launch(c, o);
    if (p.error || q.error) { CHECK(p.error == q.error, "kind %d shading %d bits %d: error %d vs %d", kind, shading, bits, (int)p.error, (int)q.error); return; }
    CHECK(p.orthographic, "kind %d shading %d bits %d override %d: not orthographic", kind, shading, bits, k);
    CHECK(!p.march.lds_staged && !p.march.deep, "kind %d shading %d bits %d: LDS staging %d, deep %d", kind, shading, bits, (int)p.march.lds_staged, (int)p.march.deep);
    if (kind == 0) CHECK(p.march.clipped, "the march is not clipped");
    if (kind == 1) CHECK(p.project.clipped, "the projection is not clipped");
    if (kind == 2) CHECK(p.isosurface.clipped, "the isosurface kernel is not clipped");
    // the clipped frame's plan but for the shade kernel's material flag, which the view vector's twin rides on
    if (kind == 0 && p.pooled) { CHECK(p.shade.material, "the orthographic shade kernel is the material variant"); q.shade.material = true; }
    CHECK(same_but_orthographic(p, q), "kind %d shading %d bits %d override %d: not the clipped frame's plan", kind, shading, bits, k);
    CHECK(plan_variants_exist(p, g.f32_general), "kind %d shading %d bits %d override %d: the plan names a variant that does not exist", kind, shading, bits, k);
  });
}

// the predicates the kernels' static_asserts ask
static void variants()
{
  int n_march = 0, n_ortho = 0;
  for (int shade = 0; shade <= 2; ++shade)
    for (int am = 0; am <= 4; ++am)
      for (int bits = 0; bits < 256; ++bits) {
        const bool pooled = bits & 1, skip = bits & 2, lds = bits & 4, deep = bits & 8, mat = bits & 16, clip = bits & 32, cached = bits & 64, f32 = bits & 128;
        const bool plain = march_variant_exists(shade, am, pooled, skip, lds, deep, mat, clip, f32, cached);
        const bool ortho = march_variant_exists(shade, am, pooled, skip, lds, deep, mat, clip, f32, cached, true);
        n_march += plain; n_ortho += ortho;
        CHECK(ortho == (plain && clip), "march shade %d am %d bits %d: the orthographic variant exists %d, the clipped one %d", shade, am, bits, (int)ortho, (int)(plain && clip));
        if (ortho) CHECK(!lds && !deep, "an orthographic LDS-staged or deep march");
      }
  CHECK(n_march > n_ortho && n_ortho > 0, "%d / %d", n_march, n_ortho);
  for (int shade = 0; shade <= 3; ++shade)
    for (int am = 0; am <= 4; ++am)
      for (int bits = 0; bits < 16; ++bits) {
        const bool skip = bits & 1, mat = bits & 2, clip = bits & 4, cached = bits & 8;
        const bool plain = shade_variant_exists(shade, am, skip, mat, clip, cached), ortho = shade_variant_exists(shade, am, skip, mat, clip, cached, true);
        CHECK(ortho == (plain && mat && clip == (shade == 2)), "shade %d am %d bits %d: %d", shade, am, bits, (int)ortho);
      }
  for (int mode = 0; mode <= 4; ++mode)
    for (int am = 0; am <= 4; ++am)
      for (int bits = 0; bits < 4; ++bits)
        CHECK(project_variant_exists(mode, am, bits & 1, bits & 2, true) == (project_variant_exists(mode, am, bits & 1, bits & 2) && (bits & 2)), "projection mode %d am %d bits %d", mode, am, bits);
  for (int shade = 0; shade <= 3; ++shade)
    for (int am = 0; am <= 4; ++am)
      for (int bits = 0; bits < 4; ++bits)
        CHECK(isosurface_variant_exists(shade, am, bits & 1, bits & 2, true) == (isosurface_variant_exists(shade, am, bits & 1, bits & 2) && (bits & 2)), "isosurface shade %d am %d bits %d", shade, am, bits);
}

int main(int argc, char** argv)
{
  struct { const char* name; void (*fn)(); } const scenarios[] = { { "off_changes_nothing", off_changes_nothing }, { "orthographic_plans", orthographic_plans }, { "variants", variants } };
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const auto& s : scenarios) printf("%s\n", s.name);
    return 0;
  }
  for (const auto& s : scenarios)
    if (argc == 2 && !strcmp(argv[1], s.name)) {
      s.fn();
      printf("%s: %d failed\n", s.name, g_failed);
      return g_failed ? 1 : 0;
    }
  printf("unknown scenario\n");
  return 2;
}
