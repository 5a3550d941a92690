// Driver of tests/test_projection_plan.py: the projection part of csrc/host/launch_plan.hpp on the CPU.  `driver <scenario>` exits 0 when every row of the
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

// projection == 0: the fields the projections added do not move a plan, and its projection part stays empty
static void off_changes_nothing()
{
  int n = 0;
  for (int shading = 0; shading <= 2; ++shading)
    for (int bits = 0; bits < 128; ++bits)
      for (int k = -1; k <= 3; ++k) {
        LaunchFacts f = small(bits & 64 ? 2 : 4);
        f.shading = shading;
        f.pool = bits & 1; f.skipping = bits & 2; f.sparse = bits & 4; f.clip_on = bits & 8; f.lds_staging = bits & 16; f.reference_material = !(bits & 32);
        f.shadow_cache = (bits & 3) == 3;
        const LaunchPlan a = plan_launch(f, ov(k));
        f.ranges = true; // bound or not: only a projection reads them
        const LaunchPlan b = plan_launch(f, ov(k));
        CHECK(same_plan(a, b), "shading %d bits %d override %d: the plan moved with `ranges`", shading, bits, k);
        CHECK(b.project.mode == 0 && !b.project.skip && !b.project.clipped && b.project.lds_bytes == 0, "shading %d bits %d: a projection part without a projection", shading, bits);
        ++n;
      }
  CHECK(n == 3 * 128 * 5, "%d plans", n);
  // two plans as literals: the unshaded in-place march, the pooled shaded one (tables 4 * (40 + 33 + 3 + 18 + 2) = 384, TF 256 * 20 + 32 = 5152)
  LaunchFacts f = small();
  LaunchPlan p = plan_launch(f);
  CHECK(!p.error && p.shading == 0 && p.am == 0 && !p.pooled && p.march_lds_bytes == 5152 + 384, "unshaded: lds %zu", p.march_lds_bytes);
  f.shading = 2; f.pool = true;
  p = plan_launch(f);
  CHECK(!p.error && p.pooled && p.march_lds_bytes == 4 * 128 * 32 + 384 + 256 * 4 + 64 && p.shade_lds_bytes == 5152 + 384 && p.shade_grid_blocks == 1024, "pooled: lds %zu / %zu", p.march_lds_bytes, p.shade_lds_bytes);
}

static void rows()
{
  // mode, ranges bound, clip box, element size, stored bytes, row_loads, override -> skip, clipped, am, lds bytes
  struct Row { const char* what; int mode; bool ranges, clip; int elem; u64 bytes; int row_loads, k; bool skip, clipped; int am; size_t lds; };
  const Row t[] = {
    { "maximum", 1, false, false, 4, 1u << 20, 0, -1, false, false, 0, 384 },
    { "maximum, ranges", 1, true, false, 4, 1u << 20, 0, -1, true, false, 0, 384 },
    { "minimum, ranges, clipped", 2, true, true, 4, 1u << 20, 0, -1, true, true, 0, 384 },
    { "mean never skips", 3, true, false, 4, 1u << 20, 0, -1, false, false, 0, 384 },
    { "mean, clipped", 3, false, true, 4, 1u << 20, 0, -1, false, true, 0, 384 },
    { "element offsets", 1, true, false, 4, GiB4 + 4, 0, -1, true, false, 1, 384 },
    { "64-bit z table: 8 * 20 + 4 * 76 = 464", 1, false, false, 4, 4 * 0xffffffffull, 0, -1, false, false, 2, 464 },
    { "computed offsets: no tables, the counters' 128 bytes", 2, true, false, 4, 1u << 20, 0, 3, true, false, 3, 128 },
    { "override 1", 3, false, false, 4, 1u << 20, 0, 1, false, false, 1, 384 },
    { "16-bit, small: 4-byte pairs", 1, false, false, 2, 1u << 20, 0, -1, false, false, 0, 384 },
    { "16-bit past 128 MiB: row loads", 1, true, false, 2, (128ull << 20) + 2, 0, -1, true, false, 4, 384 },
    { "8-bit, row loads forced", 2, false, true, 1, 1u << 20, 2, -1, false, true, 4, 384 },
    { "32-bit voxels never take the row loads", 1, false, false, 4, 1u << 20, 2, -1, false, false, 0, 384 },
    { "row loads on mode 0 only", 1, false, false, 2, 1u << 20, 2, 1, false, false, 1, 384 },
  };
  for (const Row& r : t) {
    LaunchFacts f = small(r.elem);
    f.projection = r.mode; f.ranges = r.ranges; f.clip_on = r.clip; f.stored_bytes = r.bytes; f.row_loads = r.row_loads;
    // what a projection frame ignores: shading, the pool, the majorants, LDS staging, the material
    f.shading = 2; f.pool = true; f.skipping = true; f.lds_staging = true; f.reference_material = false; f.shadow_cache = true; f.shade_order = true;
    const LaunchPlan p = plan_launch(f, ov(r.k));
    CHECK(!p.error && p.project.mode == r.mode && p.project.skip == r.skip && p.project.clipped == r.clipped && p.am == r.am && p.project.lds_bytes == r.lds,
          "%s: error %d mode %d skip %d clipped %d am %d lds %zu", r.what, (int)p.error, p.project.mode, (int)p.project.skip, (int)p.project.clipped, p.am, p.project.lds_bytes);
    CHECK(!p.pooled && !p.skip && !p.cached && !p.march.lds_staged && !p.march.deep && !p.march.material && !p.shade_order && p.shading == 0, "%s: a projection frame took part of the march's plan", r.what);
    CHECK(project_variant_exists(p.project.mode, p.am, p.project.skip, p.project.clipped), "%s: the plan names a variant that does not exist", r.what);
  }
}

static void errors()
{
  LaunchFacts f = small();
  f.projection = 4;
  CHECK(plan_launch(f).error, "mode 4");
  f.projection = -1;
  CHECK(plan_launch(f).error, "mode -1");
  f.projection = 1;
  CHECK(!plan_launch(f).error, "mode 1");
  f.tables = false;
  for (int k = 0; k <= 3; ++k) CHECK(plan_launch(f, ov(k)).error == (k < 3), "no tables at mode %d", k);
  f.tables = true; f.schedule = false;
  CHECK(plan_launch(f).error, "a dense frame without its block list");
  f.sparse = true;
  CHECK(!plan_launch(f).error, "a sparse frame needs no block list");
  f.sparse = false; f.n_schedule = 0;
  CHECK(!plan_launch(f).error, "nothing to launch");
  f.schedule = true; f.n_schedule = 20; f.quad = true;
  CHECK(plan_launch(f).error, "a quad replica: the projections read the general layout");
  // a transfer function too large to stage does not stop a projection: it reads the tables from global memory
  f.quad = false; f.n_color = f.n_alpha = 8192;
  CHECK(!plan_launch(f).error, "a transfer function of 160 KiB");
  f.projection = 0;
  CHECK(plan_launch(f).error, "... which the march cannot stage");
}

static void variants()
{
  // the combinations project_kernel's static_assert accepts: modes 1 ... 3, addressing 0 ... 4, skip for the extrema alone, either box test
  int n = 0;
  for (int mode = -1; mode <= 5; ++mode)
    for (int am = -1; am <= 5; ++am)
      for (int skip = 0; skip <= 1; ++skip)
        for (int clipped = 0; clipped <= 1; ++clipped) {
          const bool want = mode >= 1 && mode <= 3 && am >= 0 && am <= 4 && !(skip && mode == 3);
          CHECK(project_variant_exists(mode, am, skip != 0, clipped != 0) == want, "mode %d am %d skip %d clipped %d", mode, am, skip, clipped);
          n += want;
        }
  CHECK(n == 3 * 5 * 2 * 2 - 5 * 2, "%d variants", n);
  static_assert(project_variant_exists(kProjectMaximum, 0, true, false) && !project_variant_exists(kProjectMean, 0, true, false), "usable in a static_assert");
  static_assert(kProjectMaximum == 1 && kProjectMinimum == 2 && kProjectMean == 3 && kProjectK == 4, "include/ovr_hip.h's modes; the unshaded march's round");
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
