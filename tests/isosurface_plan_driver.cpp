// Driver of tests/test_isosurface_plan.py: the isosurface part of csrc/host/launch_plan.hpp on the CPU.  `driver <scenario>` exits 0 when every row of the
// scenario's table gave what the row expects; the expectations are literals, worked out by hand per row.
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

// a 40 x 33 x 18 volume of the general f32 layout under a 256 / 256 transfer function: mode 0
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
static LaunchOverrides ov(int addressing) { LaunchOverrides o; o.addressing = addressing; return o; }

// isosurfaces == 0: no plan - the march's or a projection's - has an isosurface part, and two of them are what they were, as literals
static void off_changes_nothing()
{
  int n = 0;
  for (int projection = 0; projection <= 3; ++projection)
    for (int shading = 0; shading <= 2; ++shading)
      for (int bits = 0; bits < 256; ++bits)
        for (int k = -1; k <= 3; ++k) {
          LaunchFacts f = small(bits & 64 ? 2 : 4);
          f.shading = shading; f.projection = projection;
          f.pool = bits & 1; f.skipping = bits & 2; f.sparse = bits & 4; f.clip_on = bits & 8; f.lds_staging = bits & 16; f.reference_material = !(bits & 32);
          f.ranges = bits & 128;
          f.shadow_cache = (bits & 3) == 3;
          const LaunchPlan a = plan_launch(f, ov(k));
          CHECK(!a.isosurface.on && !a.isosurface.skip && !a.isosurface.clipped && a.isosurface.lds_bytes == 0, "projection %d shading %d bits %d: an isosurface part without isovalues",
                projection, shading, bits);
          // the same facts through the two planners that existed before: plan_launch still only chooses between them
          if (projection != 0) CHECK(same_plan(a, plan_projection(f, ov(k))), "projection %d shading %d bits %d override %d", projection, shading, bits, k);
          ++n;
        }
  CHECK(n == 4 * 3 * 256 * 5, "%d plans", n);
  // (tables 4 * (40 + 33 + 3 + 18 + 2) = 384, TF 256 * 20 + 32 = 5152)
  LaunchFacts f = small();
  LaunchPlan p = plan_launch(f);
  CHECK(!p.error && p.shading == 0 && p.am == 0 && !p.pooled && p.march_lds_bytes == 5152 + 384 && p.project.mode == 0, "unshaded: lds %zu", p.march_lds_bytes);
  f.shading = 2; f.pool = true;
  p = plan_launch(f);
  CHECK(!p.error && p.pooled && p.march_lds_bytes == 4 * 128 * 32 + 384 + 256 * 4 + 64 && p.shade_lds_bytes == 5152 + 384 && p.shade_grid_blocks == 1024, "pooled: lds %zu / %zu", p.march_lds_bytes, p.shade_lds_bytes);
  f = small(); f.projection = 1; f.ranges = true;
  p = plan_launch(f);
  CHECK(!p.error && p.project.mode == 1 && p.project.skip && p.project.lds_bytes == 384 && p.march_lds_bytes == 384, "maximum: lds %zu", p.project.lds_bytes);
}

static void rows()
{
  // isovalues, shading, ranges bound, clip box, committed projection, element size, stored bytes, row_loads, override -> shading, skip, clipped, am, lds bytes
  struct Row { const char* what; int n, shading; bool ranges, clip; int projection, elem; u64 bytes; int row_loads, k; int shade; bool skip, clipped; int am; size_t lds; };
  const Row t[] = {
    { "one isovalue, unshaded", 1, 0, false, false, 0, 4, 1u << 20, 0, -1, 0, false, false, 0, 384 },
    { "gradient-shaded", 2, 1, false, false, 0, 4, 1u << 20, 0, -1, 1, false, false, 0, 384 },
    { "full shading", 4, 2, false, false, 0, 4, 1u << 20, 0, -1, 2, false, false, 0, 384 },
    { "skip only with ranges", 1, 2, true, false, 0, 4, 1u << 20, 0, -1, 2, true, false, 0, 384 },
    { "unshaded skips too", 3, 0, true, false, 0, 4, 1u << 20, 0, -1, 0, true, false, 0, 384 },
    { "the clipped variant under a clip box", 1, 1, false, true, 0, 4, 1u << 20, 0, -1, 1, false, true, 0, 384 },
    { "clipped and skipping", 1, 2, true, true, 0, 4, 1u << 20, 0, -1, 2, true, true, 0, 384 },
    { "a projection mode is ignored", 1, 2, true, false, 1, 4, 1u << 20, 0, -1, 2, true, false, 0, 384 },
    { "the mean's too (it would not skip)", 2, 0, true, true, 3, 4, 1u << 20, 0, -1, 0, true, true, 0, 384 },
    { "element offsets", 1, 2, true, false, 0, 4, GiB4 + 4, 0, -1, 2, true, false, 1, 384 },
    { "64-bit z table: 8 * 20 + 4 * 76 = 464", 1, 1, false, false, 0, 4, 4 * 0xffffffffull, 0, -1, 1, false, false, 2, 464 },
    { "computed offsets: no tables, the counters' 128 bytes", 1, 2, true, false, 2, 4, 1u << 20, 0, 3, 2, true, false, 3, 128 },
    { "16-bit, small: 4-byte pairs", 1, 0, false, false, 0, 2, 1u << 20, 0, -1, 0, false, false, 0, 384 },
    { "16-bit past 128 MiB: row loads", 1, 2, true, false, 0, 2, (128ull << 20) + 2, 0, -1, 2, true, false, 4, 384 },
    { "8-bit, row loads forced", 2, 1, false, true, 0, 1, 1u << 20, 2, -1, 1, false, true, 4, 384 },
    { "32-bit voxels never take the row loads", 1, 0, false, false, 0, 4, 1u << 20, 2, -1, 0, false, false, 0, 384 },
  };
  for (const Row& r : t) {
    LaunchFacts f = small(r.elem);
    f.isosurfaces = r.n; f.shading = r.shading; f.ranges = r.ranges; f.clip_on = r.clip; f.projection = r.projection; f.stored_bytes = r.bytes; f.row_loads = r.row_loads;
    // what an isosurface frame ignores: the pool, the majorants, LDS staging, the material (a run-time argument), the shadow cache
    f.pool = true; f.skipping = true; f.lds_staging = true; f.reference_material = false; f.shadow_cache = true; f.shade_order = true;
    const LaunchPlan p = plan_launch(f, ov(r.k));
    CHECK(!p.error && p.isosurface.on && p.shading == r.shade && p.isosurface.skip == r.skip && p.isosurface.clipped == r.clipped && p.am == r.am && p.isosurface.lds_bytes == r.lds
              && p.march_lds_bytes == r.lds,
          "%s: error %d on %d shading %d skip %d clipped %d am %d lds %zu", r.what, (int)p.error, (int)p.isosurface.on, p.shading, (int)p.isosurface.skip, (int)p.isosurface.clipped, p.am,
          p.isosurface.lds_bytes);
    CHECK(p.project.mode == 0 && !p.project.skip && !p.pooled && !p.skip && !p.cached && !p.march.lds_staged && !p.march.deep && !p.march.material && !p.shade_order,
          "%s: an isosurface frame took part of the march's or a projection's plan", r.what);
    CHECK(isosurface_variant_exists(p.shading, p.am, p.isosurface.skip, p.isosurface.clipped), "%s: the plan names a variant that does not exist", r.what);
  }
}

static void errors()
{
  LaunchFacts f = small();
  f.isosurfaces = 5;
  CHECK(plan_launch(f).error, "five isovalues");
  f.isosurfaces = -1;
  CHECK(plan_launch(f).error, "a negative count");
  f.isosurfaces = 4;
  CHECK(!plan_launch(f).error, "four");
  f.tables = false;
  for (int k = 0; k <= 3; ++k) CHECK(plan_launch(f, ov(k)).error == (k < 3), "no tables at mode %d", k);
  f.tables = true; f.schedule = false;
  CHECK(plan_launch(f).error, "a dense frame without its block list");
  f.sparse = true;
  CHECK(!plan_launch(f).error, "a sparse frame needs no block list");
  f.sparse = false; f.schedule = true; f.quad = true;
  CHECK(plan_launch(f).error, "a quad replica: the isosurfaces read the general layout");
  // a transfer function too large to stage does not stop an isosurface frame: the colour of a hit is read from global memory
  f.quad = false; f.n_color = f.n_alpha = 8192;
  CHECK(!plan_launch(f).error, "a transfer function of 160 KiB");
  f.isosurfaces = 0;
  CHECK(plan_launch(f).error, "... which the march cannot stage");
}

static void variants()
{
  int n = 0;
  for (int shade = -1; shade <= 3; ++shade)
    for (int am = -1; am <= 5; ++am)
      for (int skip = 0; skip <= 1; ++skip)
        for (int clipped = 0; clipped <= 1; ++clipped) {
          const bool want = shade >= 0 && shade <= 2 && am >= 0 && am <= 4;
          CHECK(isosurface_variant_exists(shade, am, skip != 0, clipped != 0) == want, "shade %d am %d skip %d clipped %d", shade, am, skip, clipped);
          n += want;
        }
  CHECK(n == 3 * 5 * 2 * 2, "%d variants", n);
  static_assert(isosurface_variant_exists(2, 4, true, true) && !isosurface_variant_exists(3, 0, false, false), "usable in a static_assert");
  static_assert(kMaxIsovalues == 4, "include/ovr_hip.h OVR_HIP_MAX_ISOVALUES");
}

int main(int argc, char** argv)
{
  struct S { const char* name; void (*run)(); };
  const S all[] = { { "off_changes_nothing", off_changes_nothing }, { "rows", rows }, { "errors", errors }, { "variants", variants } };
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
