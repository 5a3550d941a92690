// Driver of tests/test_shadow_cache_model.py: runs the shadow cache's host rules - csrc/host/launch_plan.hpp (which kernels a cached frame takes) and
// csrc/host/policy.hpp (the lattice's dimensions) - on the CPU.  `driver <scenario>` exits 0 when every row of the scenario gave what it expects.
// The expectations are literals worked out from DESIGN.md section 14; none is computed by calling the headers.
#include "launch_plan.hpp"
#include "plan_compare.hpp"
#include "policy.hpp"

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

static LaunchFacts f32_24()
{
  LaunchFacts f;
  f.elem_bytes = 4; f.f32_general = true;
  f.nx = f.ny = f.nz = 24;
  f.stored_bytes = 1u << 20;
  f.n_color = f.n_alpha = 256;
  f.n_blocks_owned = f.n_schedule = 96;
  return f;
}

// the cached plan: kernel SHADE 1, the material flag wherever the kernel shades, no shade order, no clipped shade variant - whatever the material, the
// clip box and the skipping are; the march keeps its clipped primary rays
static void cached_plans()
{
  struct Row { bool pool, reference, clip, skipping, order; };
  for (int bits = 0; bits < 32; ++bits) {
    const Row r = { (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0 };
    LaunchFacts f = f32_24();
    f.shading = 2; f.shadow_cache = true; f.pool = r.pool; f.reference_material = r.reference; f.clip_on = r.clip; f.skipping = r.skipping; f.shade_order = r.order;
    f.lds_staging = true;
    const LaunchPlan p = plan_launch(f);
    CHECK(!p.error && p.cached && p.shading == 1 && p.pooled == r.pool && p.skip == r.skipping, "bits %d: cached %d shading %d pooled %d", bits, (int)p.cached, p.shading, (int)p.pooled);
    CHECK(!p.shade_order && !p.shade.clipped && !p.march.lds_staged && !p.march.deep, "bits %d: order %d shade clipped %d", bits, (int)p.shade_order, (int)p.shade.clipped);
    CHECK(p.march.clipped == r.clip, "bits %d: march clipped %d", bits, (int)p.march.clipped);
    if (r.pool) CHECK(p.shade.material && !p.march.material, "bits %d: pooled: shade material %d march material %d", bits, (int)p.shade.material, (int)p.march.material);
    else CHECK(p.march.material, "bits %d: in place: march material %d", bits, (int)p.march.material);
    // LDS: the gradient-shaded frame's (in place: TF 5152 + tables 320 + queues 32768; pooled: 17792 / 5472)
    if (r.pool) CHECK(p.march_lds_bytes == 17792u && p.shade_lds_bytes == 5472u, "bits %d: %zu / %zu bytes", bits, p.march_lds_bytes, p.shade_lds_bytes);
    else CHECK(p.march_lds_bytes == 38240u, "bits %d: %zu bytes", bits, p.march_lds_bytes);
  }
  // the cache is read by full shading alone: shading NONE and GRADIENT ignore the fact
  for (int shading = 0; shading <= 1; ++shading)
    for (int pool = 0; pool <= 1; ++pool) {
      LaunchFacts f = f32_24();
      f.shading = shading; f.shadow_cache = true; f.pool = pool;
      const LaunchPlan p = plan_launch(f);
      CHECK(!p.cached && p.shading == shading && !p.march.material && !p.shade.material, "shading %d pool %d: cached %d material %d", shading, pool, (int)p.cached, (int)p.march.material);
    }
  // a small image shard: the pooled march of a cached frame may take the deep rounds like any pooled march (it does not shade)
  LaunchFacts f = f32_24();
  f.shading = 2; f.shadow_cache = true; f.pool = true; f.world = 2;
  CHECK(plan_launch(f).march.deep && plan_launch(f).cached, "a cached shard: deep %d", (int)plan_launch(f).march.deep);
}

// the launcher as it was before the fact existed, restated on the facts (tests/launch_plan_driver.cpp holds plan_launch to the same restatement)
struct Launched { int shade; bool pooled, lds_staged, deep, material, clipped, shade_material, shade_clipped, order; };
static Launched launcher_as_it_was(const LaunchFacts& f, const LaunchOverrides& o, int am)
{
  Launched l = {};
  l.shade = f.shading == 0 || f.shading == 1 ? f.shading : 2;
  l.pooled = l.shade != 0 && f.pool;
  if (!l.pooled) {
    if (f.f32_general && l.shade == 0 && am <= 1 && !f.skipping && f.lds_staging && !f.sparse && !f.clip_on) { l.lds_staged = true; return l; }
    if (f.clip_on) { l.clipped = true; l.material = l.shade != 0; }
    else if (l.shade != 0 && !f.reference_material) l.material = true;
    return l;
  }
  l.order = l.shade == 2 && f.shade_order;
  if (!f.skipping && (am <= 1 || am == 4)) {
    bool deep = f.sparse ? f.world == 1 && f.sparse_hint_pixels > 0 && f.sparse_hint_pixels <= 640000 : f.world > 1 && f.n_blocks_owned <= 10000;
    if (o.deep >= 0) deep = o.deep != 0;
    if (deep && !f.clip_on) l.deep = true;
  }
  if (!l.deep) l.clipped = f.clip_on;
  l.shade_material = !f.reference_material;
  if (l.shade == 2 && f.clip_on) l.shade_material = l.shade_clipped = true;
  return l;
}

// every plan x the fact: false -> the parent's plan (the restatement above, and `cached` clear); true -> a plan whose variants exist, equal to the plan
// of the fact-false frame wherever the shading is not the full one
static void sweep()
{
  long plans = 0, cached = 0;
  for (int bits = 0; bits < (1 << 10); ++bits)
    for (int shading = 0; shading <= 2; ++shading)
      for (int mode = 0; mode <= 4; ++mode)
        for (int elem = 1; elem <= 4; elem *= 2)
          for (int quad = 0; quad <= 1; ++quad)
            for (int shard = 0; shard <= 1; ++shard) {
              LaunchFacts f = f32_24();
              f.tables = true; f.pool = bits & 2; f.skipping = bits & 4; f.sparse = bits & 8; f.clip_on = bits & 16; f.lds_staging = bits & 32;
              f.reference_material = bits & 64; f.shade_order = bits & 128; f.schedule = true;
              const bool general = bits & 512;
              f.elem_bytes = elem; f.quad = quad; f.f32_general = general && elem == 4 && !quad;
              f.shading = shading;
              f.world = shard ? 2 : 1; f.sparse_hint_pixels = shard ? 0 : 5000;
              int expect_am = mode;
              if (mode == 1 && elem > 1) f.stored_bytes = GiB4 + 4;
              if (mode == 2) f.stored_bytes = elem == 1 ? GiB4 + 1 : (u64)elem * 0xffffffffull;
              if (mode == 3) { f.nx = 24000; f.n_color = f.n_alpha = 4096; }
              f.row_loads = mode == 4 ? 2 : 1;
              if (mode == 4 && (elem == 4 || quad)) expect_am = 0;
              LaunchOverrides o;
              o.addressing = mode == 1 && elem == 1 ? 1 : -1;
              const LaunchPlan p0 = plan_launch(f, o);
              const Launched l = launcher_as_it_was(f, o, expect_am);
              CHECK(!p0.error && !p0.cached && p0.am == expect_am && p0.shading == l.shade && p0.pooled == l.pooled && p0.march.lds_staged == l.lds_staged && p0.march.deep == l.deep
                      && p0.march.material == l.material && p0.march.clipped == l.clipped,
                    "bits %d shading %d mode %d elem %d quad %d shard %d: the plan without the fact moved", bits, shading, mode, elem, quad, shard);
              if (p0.pooled) CHECK(p0.shade.material == l.shade_material && p0.shade.clipped == l.shade_clipped && p0.shade_order == l.order, "bits %d shading %d: shade", bits, shading);
              CHECK(march_variant_exists(p0.shading, p0.am, p0.pooled, p0.skip, p0.march.lds_staged, p0.march.deep, p0.march.material, p0.march.clipped, f.f32_general, false),
                    "bits %d shading %d mode %d: no such march variant without the fact", bits, shading, mode);
              f.shadow_cache = true;
              const LaunchPlan p1 = plan_launch(f, o);
              ++plans;
              if (shading != 2) { CHECK(same_plan(p0, p1) && !p1.cached, "bits %d shading %d mode %d: the fact moved a plan that does not read the cache", bits, shading, mode); continue; }
              ++cached;
              CHECK(!p1.error && p1.cached && p1.shading == 1 && p1.am == p0.am && p1.pooled == p0.pooled && p1.skip == p0.skip, "bits %d mode %d: cached plan", bits, mode);
              CHECK(march_variant_exists(p1.shading, p1.am, p1.pooled, p1.skip, p1.march.lds_staged, p1.march.deep, p1.march.material, p1.march.clipped, f.f32_general,
                                         p1.cached && !p1.pooled),
                    "bits %d mode %d elem %d quad %d shard %d: no such cached march variant", bits, mode, elem, quad, shard);
              if (p1.pooled)
                CHECK(shade_variant_exists(p1.shading, p1.am, p1.skip, p1.shade.material, p1.shade.clipped, true) && !p1.shade_order, "bits %d mode %d: no such cached shade variant", bits, mode);
            }
  printf("sweep: %ld plans, %ld cached\n", plans, cached);
  CHECK(plans == 1024L * 3 * 5 * 3 * 2 * 2 && cached == plans / 3, "the sweep's size");
  // the predicates: a cached variant exists only where the kernel shades without a shadow march, on the material variant
  CHECK(march_variant_exists(1, 0, false, false, false, false, true, false, true, true), "the cached in-place march");
  CHECK(march_variant_exists(1, 3, false, true, false, false, true, true, false, true), "the cached clipped skipping in-place march at mode 3");
  CHECK(!march_variant_exists(2, 0, false, false, false, false, true, false, true, true), "a cached march with a shadow march exists");
  CHECK(!march_variant_exists(1, 0, false, false, false, false, false, false, true, true), "a cached march without the material exists");
  CHECK(!march_variant_exists(1, 0, true, false, false, false, false, false, true, true), "a cached pooled march exists");
  CHECK(!march_variant_exists(0, 0, false, false, true, false, false, false, true, true), "a cached LDS-staged march exists");
  CHECK(!march_variant_exists(0, 0, false, false, false, false, false, false, true, true), "a cached unshaded march exists");
  CHECK(shade_variant_exists(1, 0, false, true, false, true) && shade_variant_exists(1, 4, true, true, false, true), "the cached shade kernel");
  CHECK(!shade_variant_exists(2, 0, false, true, false, true), "a cached shade kernel with a shadow march exists");
  CHECK(!shade_variant_exists(1, 0, false, false, false, true), "a cached shade kernel without the material exists");
  CHECK(!shade_variant_exists(1, 0, false, true, true, true), "a cached clipped shade kernel exists");
}

// the lattice's dimensions.  (When a built lattice is stale is a column of csrc/host/commit_plan.hpp's table: the staleness table that stood here - each
// change alone, and together with every change that does not count - is tests/commit_plan_driver.cpp's scenario shadow_staleness, expectations intact.)
static void staleness()
{
  // lattice dimensions: ceil(dim / cell) + 1
  CHECK(policy::shadow_cache_nodes(32, 2) == 17 && policy::shadow_cache_nodes(32, 4) == 9 && policy::shadow_cache_nodes(40, 3) == 15 && policy::shadow_cache_nodes(20, 3) == 8
          && policy::shadow_cache_nodes(1, 4) == 2 && policy::shadow_cache_nodes(1024, 1) == 1025 && policy::shadow_cache_nodes(33, 32) == 3,
        "nodes per axis");
  CHECK(policy::kShadowCacheDefaultCell == 4, "the default cell");
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "cached_plans", cached_plans }, { "sweep", sweep }, { "staleness", staleness } };

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const Scenario& s : kScenarios) printf("%s\n", s.name);
    return 0;
  }
  for (const Scenario& s : kScenarios)
    if (argc == 2 && !strcmp(argv[1], s.name)) {
      s.run();
      printf("%s: %s\n", s.name, g_failed ? "FAILED" : "ok");
      return g_failed ? 1 : 0;
    }
  printf("usage: driver --list | <scenario>\n");
  return 2;
}
