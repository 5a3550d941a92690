// Driver of tests/test_slices_plan.py: the slice part of csrc/host/launch_plan.hpp and the commit plan's row of the frame kinds on the CPU.  `driver <scenario>`
// exits 0 when every row of the scenario's table gave what the row expects; the expectations are literals, worked out by hand per row.
#include "commit_plan.hpp"
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
static LaunchOverrides ov(int addressing) { LaunchOverrides o; o.addressing = addressing; return o; }

// plane versus walk kernel; the skipping twin only with bound ranges and an extremum slab; the clipped / orthographic twins by the projection's rule
static void kernels()
{
  // (tables 4 * (40 + 33 + 3 + 18 + 2) = 384 bytes: the only LDS of a walk frame)
  LaunchFacts f = small();
  f.slices = 1;
  LaunchPlan p = plan_launch(f);
  CHECK(!p.error && p.slices.on && !p.slices.walks && !p.slices.skip && !p.slices.clipped && p.am == 0 && p.march_lds_bytes == 384 && p.slices.lds_bytes == 384, "one plane: lds %zu", p.march_lds_bytes);
  CHECK(!p.pooled && !p.skip && p.project.mode == 0 && !p.isosurface.on && p.shade_grid_blocks == 0 && plan_variants_exist(p, true), "one plane: nothing else of the plan is set");
  f.ranges = true; // planes fetch everything: no twin, whatever is bound
  p = plan_launch(f);
  CHECK(p.slices.on && !p.slices.walks && !p.slices.skip && plan_variants_exist(p, true), "planes with ranges bound");
  f.slices = 3; f.slice_walks = true; f.slice_extremum = false; // a MEAN slab among planes: the walk kernel, nothing to skip
  p = plan_launch(f);
  CHECK(p.slices.on && p.slices.walks && !p.slices.skip && plan_variants_exist(p, true), "a mean slab");
  f.slice_extremum = true;
  p = plan_launch(f);
  CHECK(p.slices.walks && p.slices.skip && plan_variants_exist(p, true), "an extremum slab with ranges");
  f.ranges = false;
  p = plan_launch(f);
  CHECK(p.slices.walks && !p.slices.skip, "an extremum slab without ranges");
  f.slice_walks = false; f.ranges = true; // (an inconsistent fact - an extremum without a slab - still gives the plane kernel without a twin)
  p = plan_launch(f);
  CHECK(!p.slices.walks && !p.slices.skip && plan_variants_exist(p, true), "no slab: no twin");
  for (int walks = 0; walks < 2; ++walks)
    for (int clip = 0; clip < 2; ++clip)
      for (int ortho = 0; ortho < 2; ++ortho) {
        LaunchFacts g = small();
        g.slices = 2; g.slice_walks = walks; g.slice_extremum = walks; g.ranges = true; g.clip_on = clip; g.orthographic = ortho;
        p = plan_launch(g);
        CHECK(p.slices.on && p.slices.clipped == (clip || ortho) && p.orthographic == (ortho != 0) && p.slices.skip == (walks != 0) && plan_variants_exist(p, true),
              "walks %d clip %d ortho %d", walks, clip, ortho);
      }
  // the addressing modes: the layout's, a more general one on request, the row loads on the 16-bit layouts
  for (int k = 0; k <= 3; ++k) {
    p = plan_launch(f, ov(k));
    CHECK(p.am == k && p.march_lds_bytes == (k == 3 ? 128u : k == 2 ? 464u : 384u), "addressing %d: am %d lds %zu", k, p.am, p.march_lds_bytes);
  }
  LaunchFacts h = small(2);
  h.slices = 1; h.row_loads = 2;
  p = plan_launch(h);
  CHECK(p.am == 4 && plan_variants_exist(p, false), "row loads: am %d", p.am);
  // errors: more than four slices, a quad replica's layout, missing tables
  f = small(); f.slices = 5;
  CHECK(plan_launch(f).error, "five slices");
  f.slices = 1; f.quad = true;
  CHECK(plan_launch(f).error, "a quad layout");
  f.quad = false; f.tables = false;
  CHECK(plan_launch(f).error, "no tables");
  CHECK(!slice_variant_exists(false, 0, true, false) && !slice_variant_exists(true, 5, false, false) && slice_variant_exists(true, 0, true, false), "the predicate");
}

// slices draw whatever isovalues and projection mode are committed; shading, pool, majorants and LDS staging are not read
static void precedence()
{
  int n = 0;
  for (int projection = 0; projection <= 3; ++projection)
    for (int iso = 0; iso <= 4; ++iso)
      for (int shading = 0; shading <= 2; ++shading)
        for (int bits = 0; bits < 64; ++bits) {
          LaunchFacts f = small();
          f.projection = projection; f.isosurfaces = iso; f.shading = shading;
          f.pool = bits & 1; f.skipping = bits & 2; f.lds_staging = bits & 4; f.translucent = iso > 0 && (bits & 8); f.ambient_occlusion = iso > 0 && (bits & 16);
          f.shadow_cache = bits & 32;
          f.slices = 2; f.slice_walks = true; f.slice_extremum = true; f.ranges = true;
          LaunchFacts g = small();
          g.slices = 2; g.slice_walks = true; g.slice_extremum = true; g.ranges = true;
          const LaunchPlan a = plan_launch(f), b = plan_launch(g);
          CHECK(a.slices.on && a.project.mode == 0 && !a.isosurface.on && !a.ambient_occlusion && !a.pooled && !a.skip && !a.cached && a.shading == 0 && same_plan(a, b),
                "projection %d isovalues %d shading %d bits %d", projection, iso, shading, bits);
          ++n;
        }
  CHECK(n == 4 * 5 * 3 * 64, "%d plans", n);
}

// slices == 0: no plan has a slice part, and every plan is the one the three planners that existed before give
static void off_changes_nothing()
{
  int n = 0;
  for (int projection = 0; projection <= 3; ++projection)
    for (int iso = 0; iso <= 2; ++iso)
      for (int shading = 0; shading <= 2; ++shading)
        for (int bits = 0; bits < 512; ++bits)
          for (int k = -1; k <= 3; ++k) {
            LaunchFacts f = small(bits & 64 ? 2 : 4);
            f.shading = shading; f.projection = projection; f.isosurfaces = iso;
            f.pool = bits & 1; f.skipping = bits & 2; f.sparse = bits & 4; f.clip_on = bits & 8; f.lds_staging = bits & 16; f.reference_material = !(bits & 32);
            f.ranges = bits & 128; f.orthographic = bits & 256;
            f.slice_walks = true; f.slice_extremum = true; // (facts of slices that are not committed are not read)
            const LaunchPlan a = plan_launch(f, ov(k));
            CHECK(!a.slices.on && !a.slices.walks && !a.slices.skip && !a.slices.clipped && a.slices.lds_bytes == 0, "projection %d isovalues %d shading %d bits %d: a slice part without slices",
                  projection, iso, shading, bits);
            if (iso != 0) CHECK(same_plan(a, plan_isosurface(f, ov(k))), "isovalues: projection %d shading %d bits %d override %d", projection, shading, bits, k);
            else if (projection != 0) CHECK(same_plan(a, plan_projection(f, ov(k))), "projection %d shading %d bits %d override %d", projection, shading, bits, k);
            ++n;
          }
  CHECK(n == 4 * 3 * 3 * 512 * 5, "%d plans", n);
  // two march plans as literals (tables 384, TF 256 * 20 + 32 = 5152): what they were before the slices
  LaunchFacts f = small();
  LaunchPlan p = plan_launch(f);
  CHECK(!p.error && p.shading == 0 && p.am == 0 && !p.pooled && p.march_lds_bytes == 5152 + 384 && p.project.mode == 0 && !p.slices.on, "unshaded: lds %zu", p.march_lds_bytes);
  f.shading = 2; f.pool = true;
  p = plan_launch(f);
  CHECK(!p.error && p.pooled && p.march_lds_bytes == 4 * 128 * 32 + 384 + 256 * 4 + 64 && p.shade_lds_bytes == 5152 + 384 && p.shade_grid_blocks == 1024 && !p.slices.on, "pooled: lds %zu / %zu",
        p.march_lds_bytes, p.shade_lds_bytes);
}

// ovr_hip_set_slices is recorded under kShading, like the projection mode and the isovalues: the accumulation starts over, nothing else is voided
static void commit_row()
{
  using namespace commit;
  Changes c;
  c.note(kShading, true, true);
  CommitFacts facts;
  facts.framebuffer = facts.volume = true;
  const Effects e = plan_commit(c, facts);
  CHECK(e.has(kReset) && e.has(kEstimateVoid) && e.has(kBumpClearGen) && e.has(kPoolUnproven), "the accumulation, the estimate that rests on it, the cleared blocks' pixels, the pool's proof: %#x", e.what);
  CHECK(e.what == kChanged, "and nothing else: %#x", e.what);
  CHECK(!e.has(kResort) && !e.has(kRelist) && !e.has(kMajorantVoid) && !e.has(kRangesVoid) && !e.has(kLatticeStale) && !e.has(kSkipRestart) && !e.has(kCameraParams)
          && !e.has(kVolumeParams) && !e.has(kLighting) && !e.has(kClipParams) && !e.has(kFreeConvergence) && !e.has(kFreeReconstruction) && !e.has(kFreeBuiltLattice)
          && !e.has(kFreeSuppliedLattice),
        "no schedule, majorant, range, lattice or parameter follows from the frame kind: %#x", e.what);
  CHECK(e.tuner == kTunerChanged, "the tuner: %d", (int)e.tuner);
  Changes same; // the same slices again: still a call - the accumulation starts over (every call resets it)
  same.note(kShading, true, false);
  CHECK(plan_commit(same, facts).what == kChanged, "the same value again");
  Changes none;
  CHECK(plan_commit(none, facts).what == 0u, "no call, no effect");
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "kernels", kernels }, { "precedence", precedence }, { "off_changes_nothing", off_changes_nothing }, { "commit_row", commit_row } };

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const Scenario& s : kScenarios) printf("%s\n", s.name);
    return 0;
  }
  for (const Scenario& s : kScenarios)
    if (argc == 2 && !strcmp(argv[1], s.name)) {
      s.run();
      if (g_failed) printf("%d checks failed\n", g_failed);
      return g_failed ? 1 : 0;
    }
  printf("usage: driver --list | <scenario>\n");
  return 2;
}
