// Driver of tests/test_slice_context_plan.py: the slice context's part of csrc/host/launch_plan.hpp and the commit plan's row of the frame kinds on the CPU.
// `driver <scenario>` exits 0 when every row of the scenario's table gave what the row expects; the expectations are literals, worked out by hand per row.
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

// the context bit, the one kernel for plane-only and slab sets, the transfer function in LDS, no skipping twin, the clipped variants alone
static void context()
{
  // tables 4 * (40 + 33 + 3 + 18 + 2) = 384 bytes; the transfer function 256 * 16 + 256 * 4 + 32 = 5152
  for (int walks = 0; walks < 2; ++walks)
    for (int extremum = 0; extremum <= walks; ++extremum)
      for (int ranges = 0; ranges < 2; ++ranges)
        for (int clip = 0; clip < 2; ++clip)
          for (int ortho = 0; ortho < 2; ++ortho) {
            LaunchFacts f = small();
            f.slices = 2; f.slice_walks = walks; f.slice_extremum = extremum; f.ranges = ranges; f.clip_on = clip; f.orthographic = ortho; f.skipping = ranges;
            f.slice_context = true;
            const LaunchPlan p = plan_launch(f);
            CHECK(!p.error && p.slices.on && p.slices.context && p.slices.walks == (walks != 0), "walks %d extremum %d ranges %d clip %d ortho %d: the bit", walks, extremum, ranges, clip, ortho);
            CHECK(!p.slices.skip && !p.skip, "walks %d extremum %d ranges %d: a context frame fetches every step", walks, extremum, ranges);
            CHECK(p.slices.clipped && p.orthographic == (ortho != 0), "clip %d ortho %d: the clipped kernel with the unit box", clip, ortho);
            CHECK(p.march_lds_bytes == 384 + 5152 && p.slices.lds_bytes == 384 + 5152, "lds %zu", p.march_lds_bytes);
            CHECK(plan_variants_exist(p, true) && slice_variant_exists(p.slices.walks, p.am, p.slices.skip, p.slices.clipped, p.orthographic, true), "the variant exists");
            CHECK(!p.pooled && p.project.mode == 0 && !p.isosurface.on && p.shade_grid_blocks == 0 && p.shading == 0, "nothing else of the plan is set");
          }
  // the addressing modes: the tables in front of the transfer function (16-byte aligned), none in mode 3; the row loads on the 16-bit layouts
  LaunchFacts f = small();
  f.slices = 1; f.slice_context = true;
  for (int k = 0; k <= 3; ++k) {
    const LaunchPlan p = plan_launch(f, ov(k));
    CHECK(p.am == k && p.march_lds_bytes == 5152u + (k == 3 ? 0u : k == 2 ? 464u : 384u), "addressing %d: am %d lds %zu", k, p.am, p.march_lds_bytes);
  }
  LaunchFacts h = small(2);
  h.slices = 1; h.slice_context = true; h.row_loads = 2;
  LaunchPlan p = plan_launch(h);
  CHECK(p.am == 4 && p.slices.context && plan_variants_exist(p, false), "row loads: am %d", p.am);
  // a tiny table still leaves room for the counter reduction's words
  f.nx = f.ny = f.nz = 1; f.n_color = f.n_alpha = 1;
  p = plan_launch(f, ov(3));
  CHECK(p.march_lds_bytes == 128 && !p.error, "mode 3, one-entry tables (16 + 4 + 32 = 52 bytes): lds %zu, the counters' 4 x 8 words", p.march_lds_bytes);
  // errors: an oversized table (tf_lds_bytes gives 0 above 96 KiB), as the march has it; the slice frame of the same facts does not read the table
  f = small(); f.slices = 2; f.slice_context = true; f.n_color = 8192; // 128 KiB of colours
  CHECK(plan_launch(f).error && !plan_launch(f).slices.on, "an oversized table");
  f.slice_context = false;
  CHECK(!plan_launch(f).error, "the slice frame does not stage it");
  f.slice_context = true; f.n_color = 256; f.slices = 5;
  CHECK(plan_launch(f).error, "five slices");
  f.slices = 1; f.quad = true;
  CHECK(plan_launch(f).error, "a quad layout");
  // the predicate: clipped alone, no skipping twin, both cameras, `walks` not read
  CHECK(slice_variant_exists(false, 0, false, true, false, true) && slice_variant_exists(true, 3, false, true, true, true) && !slice_variant_exists(true, 0, false, false, false, true)
          && !slice_variant_exists(true, 0, true, true, false, true) && !slice_variant_exists(false, 5, false, true, false, true),
        "the predicate");
}

// slices > isovalues > projection, with the context as without it; the context without slices is not read
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
          f.slices = 2; f.slice_walks = true; f.slice_extremum = true; f.ranges = true; f.slice_context = true;
          LaunchFacts g = small();
          g.slices = 2; g.slice_walks = true; g.slice_extremum = true; g.ranges = true; g.slice_context = true;
          const LaunchPlan a = plan_launch(f), b = plan_launch(g);
          CHECK(a.slices.on && a.slices.context && a.project.mode == 0 && !a.isosurface.on && !a.ambient_occlusion && !a.pooled && !a.skip && !a.cached && a.shading == 0 && same_plan(a, b),
                "projection %d isovalues %d shading %d bits %d", projection, iso, shading, bits);
          // without slices the committed context is kept and not read: the frame is the isosurface, projection or march frame it was
          f.slices = 0;
          LaunchFacts off = f;
          off.slice_context = false;
          const LaunchPlan c = plan_launch(f), d = plan_launch(off);
          CHECK(!c.slices.on && !c.slices.context && same_plan(c, d) && c.isosurface.on == (iso != 0) && c.project.mode == (iso != 0 ? 0 : projection),
                "n = 0: projection %d isovalues %d shading %d bits %d", projection, iso, shading, bits);
          ++n;
        }
  CHECK(n == 4 * 5 * 3 * 64, "%d plans", n);
}

// mode OFF: every plan is the one the facts planned before the context existed - literals for the slice frames, and no plan carries the bit
static void off_changes_nothing()
{
  int n = 0;
  for (int slices = 0; slices <= 4; ++slices)
    for (int projection = 0; projection <= 3; ++projection)
      for (int shading = 0; shading <= 2; ++shading)
        for (int bits = 0; bits < 512; ++bits)
          for (int k = -1; k <= 3; ++k) {
            LaunchFacts f = small(bits & 64 ? 2 : 4);
            f.shading = shading; f.projection = projection; f.slices = slices;
            f.pool = bits & 1; f.skipping = bits & 2; f.sparse = bits & 4; f.clip_on = bits & 8; f.lds_staging = bits & 16; f.slice_walks = bits & 32;
            f.slice_extremum = (bits & 32) && (bits & 128); f.ranges = bits & 128; f.orthographic = bits & 256;
            const LaunchPlan a = plan_launch(f, ov(k));
            CHECK(!a.slices.context, "slices %d projection %d shading %d bits %d override %d: the bit without the fact", slices, projection, shading, bits, k);
            if (slices > 0) {
              // the slice frame's plan as section 21 states it: the tables alone in LDS, the twin by ranges and an extremum slab, clipped by box or camera
              const int am = a.am;
              const size_t tables = am == 3 ? 0 : am == 2 ? (size_t)20 * 8 + 76 * 4 : (size_t)96 * 4;
              CHECK(!a.error && a.slices.on && a.slices.walks == ((bits & 32) != 0) && a.slices.skip == ((bits & 32) && (bits & 128)) && a.slices.clipped == ((bits & 8) || (bits & 256))
                      && a.march_lds_bytes == std::max<size_t>(tables, 128) && a.slices.lds_bytes == a.march_lds_bytes,
                    "slices %d bits %d override %d: lds %zu", slices, bits, k, a.march_lds_bytes);
            }
            ++n;
          }
  CHECK(n == 5 * 4 * 3 * 512 * 5, "%d plans", n);
  // the literals of tests/slices_plan_driver.cpp, again: one plane 384 bytes; the unshaded march 5152 + 384
  LaunchFacts f = small();
  f.slices = 1;
  LaunchPlan p = plan_launch(f);
  CHECK(!p.error && p.slices.on && !p.slices.context && !p.slices.clipped && p.march_lds_bytes == 384, "one plane: lds %zu", p.march_lds_bytes);
  f.slices = 0;
  p = plan_launch(f);
  CHECK(!p.error && !p.slices.on && p.march_lds_bytes == 5152 + 384, "unshaded march: lds %zu", p.march_lds_bytes);
  // the trailing default of the predicate: the five-argument calls read as before
  CHECK(slice_variant_exists(false, 0, false, false) && !slice_variant_exists(false, 0, true, true) && !slice_variant_exists(true, 0, false, false, true), "the predicate without the context");
}

// ovr_hip_set_slice_context is recorded under kShading, like the other frame kinds: the accumulation starts over, nothing else is voided
static void commit_row()
{
  using namespace commit;
  Changes c;
  c.note(kShading, true, true);
  CommitFacts facts;
  facts.framebuffer = facts.volume = true;
  const Effects e = plan_commit(c, facts);
  CHECK(e.has(kReset) && e.what == kChanged, "the accumulation starts over and nothing else follows: %#x", e.what);
  CHECK(!e.has(kResort) && !e.has(kRelist) && !e.has(kMajorantVoid) && !e.has(kRangesVoid) && !e.has(kLatticeStale) && !e.has(kSkipRestart), "nothing is voided: %#x", e.what);
  Changes same; // the same mode and scale again: still a call
  same.note(kShading, true, false);
  CHECK(plan_commit(same, facts).what == kChanged, "the same value again");
  Changes none;
  CHECK(plan_commit(none, facts).what == 0u, "no call, no effect");
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "context", context }, { "precedence", precedence }, { "off_changes_nothing", off_changes_nothing }, { "commit_row", commit_row } };

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
