// Driver of tests/test_isosurface_layers_plan.py: the translucent part of csrc/host/launch_plan.hpp (LaunchFacts::translucent, LaunchPlan::Isosurface::translucent,
// isosurface_variant_exists) on the CPU.  `driver <scenario>` exits 0 when every row of the scenario gave what it expects; the rows' expectations are literals.
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

typedef unsigned long long u64;
constexpr u64 GiB4 = 0x100000000ull;

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

// the same plan but for the translucent flag
static bool same_but_translucent(LaunchPlan a, const LaunchPlan& b)
{
  a.isosurface.translucent = b.isosurface.translucent;
  return same_plan(a, b);
}

template <typename F> static int for_all_facts(F&& fn)
{
  int n = 0;
  for (int kind = 0; kind < 3; ++kind) // the march, a projection, isosurfaces
    for (int shading = 0; shading <= 2; ++shading)
      for (int bits = 0; bits < 1024; ++bits)
        for (int k = -1; k <= 3; k += 2) {
          LaunchFacts f = small(bits & 64 ? 2 : 4);
          f.shading = shading;
          f.pool = bits & 1; f.skipping = bits & 2; f.sparse = bits & 4; f.clip_on = bits & 8; f.lds_staging = bits & 16; f.reference_material = !(bits & 32);
          f.shadow_cache = bits & 128; f.ranges = bits & 2;
          if (bits & 256) { f.world = 4; f.n_blocks_owned = 10; }
          f.orthographic = bits & 512;
          f.projection = kind == 1 ? 1 + (bits & 1) * 2 : 0; // maximum or mean
          f.isosurfaces = kind == 2 ? 1 + (bits & 3) : 0;
          fn(f, ov(k, bits & 256 ? 1 : -1), kind, shading, bits, k);
          ++n;
        }
  return n;
}

// translucent == false: no plan has a translucent part, and what decides the clipped isosurface variant is what decided it - the clip box and the camera.
// Without isovalues the fact is not read at all: the march's and a projection's plan with it are the plans without it
static void off_changes_nothing()
{
  // plans of the launcher as it was, as literals (tables 4 * (40 + 33 + 3 + 18 + 2) = 384)
  LaunchFacts f = small();
  f.isosurfaces = 2; f.shading = 2; f.ranges = true;
  LaunchPlan p = plan_launch(f);
  CHECK(!p.error && p.isosurface.on && p.isosurface.skip && !p.isosurface.clipped && !p.isosurface.translucent && p.shading == 2 && p.am == 0 && p.isosurface.lds_bytes == 384
            && p.march_lds_bytes == 384 && !p.orthographic,
        "opaque, skipping: clipped %d lds %zu", (int)p.isosurface.clipped, p.isosurface.lds_bytes);
  f.clip_on = true; f.ranges = false; f.shading = 0;
  p = plan_launch(f);
  CHECK(!p.error && p.isosurface.on && !p.isosurface.skip && p.isosurface.clipped && !p.isosurface.translucent && p.shading == 0, "opaque, clipped");
  f.clip_on = false; f.orthographic = true;
  p = plan_launch(f);
  CHECK(!p.error && p.isosurface.clipped && p.orthographic && !p.isosurface.translucent, "opaque, orthographic");
  const int n = for_all_facts([](LaunchFacts f, const LaunchOverrides& o, int kind, int shading, int bits, int k) {
    const LaunchPlan a = plan_launch(f, o);
    CHECK(!a.isosurface.translucent, "kind %d shading %d bits %d override %d: translucent without the fact", kind, shading, bits, k);
    CHECK(a.error || plan_variants_exist(a, f.f32_general), "kind %d shading %d bits %d override %d: the plan names a variant that does not exist", kind, shading, bits, k);
    if (!a.error && kind == 2) CHECK(a.isosurface.clipped == (f.clip_on || f.orthographic) && a.isosurface.skip == f.ranges, "isosurface bits %d: clipped %d skip %d", bits, (int)a.isosurface.clipped, (int)a.isosurface.skip);
    if (kind != 2) { // the fact is an isosurface frame's alone
      LaunchFacts g = f;
      g.translucent = true;
      const LaunchPlan b = plan_launch(g, o);
      CHECK(same_but_translucent(a, b) && !b.isosurface.translucent && !b.isosurface.on, "kind %d shading %d bits %d override %d: the fact changed a plan without isovalues", kind, shading, bits, k);
    }
  });
  CHECK(n == 3 * 3 * 1024 * 3, "%d plans", n);
}

// the translucent plan table
static void rows()
{
  // isovalues, shading, ranges bound, clip box, orthographic, element size, stored bytes, row_loads, override -> shading, skip, clipped, orthographic, am, lds bytes
  struct Row { const char* what; int n, shading; bool ranges, clip, ortho; int elem; u64 bytes; int row_loads, k; int shade; bool skip, clipped, orthographic; int am; size_t lds; };
  const Row t[] = {
    { "no clip box: the clipped variant with the unit box", 2, 2, false, false, false, 4, 1u << 20, 0, -1, 2, false, true, false, 0, 384 },
    { "skip as the opaque frame: with the ranges", 4, 2, true, false, false, 4, 1u << 20, 0, -1, 2, true, true, false, 0, 384 },
    { "unshaded", 1, 0, false, false, false, 4, 1u << 20, 0, -1, 0, false, true, false, 0, 384 },
    { "gradient-shaded, skipping", 3, 1, true, false, false, 4, 1u << 20, 0, -1, 1, true, true, false, 0, 384 },
    { "under a clip box", 2, 1, false, true, false, 4, 1u << 20, 0, -1, 1, false, true, false, 0, 384 },
    { "orthographic", 2, 2, true, false, true, 4, 1u << 20, 0, -1, 2, true, true, true, 0, 384 },
    { "orthographic under a clip box", 2, 0, false, true, true, 4, 1u << 20, 0, -1, 0, false, true, true, 0, 384 },
    { "element offsets", 1, 2, true, false, false, 4, GiB4 + 4, 0, -1, 2, true, true, false, 1, 384 },
    { "64-bit z table: 8 * 20 + 4 * 76 = 464", 1, 1, false, false, false, 4, 4 * 0xffffffffull, 0, -1, 1, false, true, false, 2, 464 },
    { "computed offsets: no tables, the counters' 128 bytes", 1, 2, true, false, false, 4, 1u << 20, 0, 3, 2, true, true, false, 3, 128 },
    { "16-bit past 128 MiB: row loads", 1, 2, true, false, false, 2, (128ull << 20) + 2, 0, -1, 2, true, true, false, 4, 384 },
    { "8-bit, row loads forced", 2, 1, false, true, false, 1, 1u << 20, 2, -1, 1, false, true, false, 4, 384 },
  };
  for (const Row& r : t) {
    LaunchFacts f = small(r.elem);
    f.isosurfaces = r.n; f.translucent = true; f.shading = r.shading; f.ranges = r.ranges; f.clip_on = r.clip; f.orthographic = r.ortho; f.stored_bytes = r.bytes; f.row_loads = r.row_loads;
    f.pool = true; f.skipping = true; f.lds_staging = true; f.reference_material = false; f.shadow_cache = true; f.shade_order = true; f.projection = 1; // all ignored
    const LaunchPlan p = plan_launch(f, ov(r.k));
    CHECK(!p.error && p.isosurface.on && p.isosurface.translucent && p.shading == r.shade && p.isosurface.skip == r.skip && p.isosurface.clipped == r.clipped
              && p.orthographic == r.orthographic && p.am == r.am && p.isosurface.lds_bytes == r.lds && p.march_lds_bytes == r.lds,
          "%s: error %d translucent %d shading %d skip %d clipped %d ortho %d am %d lds %zu", r.what, (int)p.error, (int)p.isosurface.translucent, p.shading, (int)p.isosurface.skip,
          (int)p.isosurface.clipped, (int)p.orthographic, p.am, p.isosurface.lds_bytes);
    CHECK(p.project.mode == 0 && !p.pooled && !p.skip && !p.cached && !p.march.lds_staged && !p.march.deep && !p.march.material && !p.shade_order,
          "%s: a translucent frame took part of the march's or a projection's plan", r.what);
    CHECK(plan_variants_exist(p, f.f32_general), "%s: the plan names a variant that does not exist", r.what);
  }
}

// a translucent frame's plan IS the plan of the same opaque frame under a clip box, with the translucent flag; the error cases are the opaque frame's
static void sweep()
{
  int seen = 0;
  for_all_facts([&](LaunchFacts f, const LaunchOverrides& o, int kind, int shading, int bits, int k) {
    if (kind != 2) return;
    LaunchFacts g = f;
    g.translucent = true;
    const LaunchPlan p = plan_launch(g, o);
    LaunchFacts c = f;
    c.clip_on = true;
    const LaunchPlan q = plan_launch(c, o);
    if (p.error || q.error) { CHECK(p.error == q.error, "shading %d bits %d: error %d vs %d", shading, bits, (int)p.error, (int)q.error); return; }
    CHECK(p.isosurface.translucent && p.isosurface.clipped && p.isosurface.skip == f.ranges, "shading %d bits %d override %d: translucent %d clipped %d", shading, bits, k,
          (int)p.isosurface.translucent, (int)p.isosurface.clipped);
    CHECK(same_but_translucent(p, q), "shading %d bits %d override %d: not the clipped frame's plan", shading, bits, k);
    CHECK(plan_variants_exist(p, g.f32_general) && isosurface_variant_exists(p.shading, p.am, p.isosurface.skip, p.isosurface.clipped, p.orthographic, true),
          "shading %d bits %d override %d: the plan names a variant that does not exist", shading, bits, k);
    ++seen;
  });
  CHECK(seen == 3 * 1024 * 3, "%d translucent plans", seen);
  LaunchFacts f = small();
  f.translucent = true; f.isosurfaces = 5;
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
      for (int bits = 0; bits < 8; ++bits) {
        const bool skip = bits & 1, clipped = bits & 2, ortho = bits & 4;
        const bool want = shade >= 0 && shade <= 2 && am >= 0 && am <= 4 && clipped;
        CHECK(isosurface_variant_exists(shade, am, skip, clipped, ortho, true) == want, "shade %d am %d bits %d", shade, am, bits);
        CHECK(isosurface_variant_exists(shade, am, skip, clipped, ortho, false) == isosurface_variant_exists(shade, am, skip, clipped, ortho), "the default is false");
        n += want;
      }
  CHECK(n == 3 * 5 * 2 * 2, "%d translucent variants: half of what both box tests would take", n);
  static_assert(isosurface_variant_exists(2, 4, true, true, true, true) && !isosurface_variant_exists(2, 4, true, false, false, true), "usable in a static_assert");
}

int main(int argc, char** argv)
{
  struct S { const char* name; void (*run)(); };
  const S all[] = { { "off_changes_nothing", off_changes_nothing }, { "rows", rows }, { "sweep", sweep }, { "variants", variants } };
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
