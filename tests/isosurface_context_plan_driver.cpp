// Driver of tests/test_isosurface_context_plan.py: the isosurface context's part of csrc/host/launch_plan.hpp and the commit plan's row of the frame kinds on the
// CPU.  `driver <scenario>` exits 0 when every row of the scenario's table gave what the row expects; the expectations are literals, worked out by hand per row.
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

// a context plan is the clipped translucent plan of the same facts plus the flag, with the transfer function's LDS and without skip or AO
static void context()
{
  // tables 4 * (40 + 33 + 3 + 18 + 2) = 384 bytes; the transfer function 256 * 16 + 256 * 4 + 32 = 5152
  int n = 0;
  for (int iso = 1; iso <= 4; ++iso)
    for (int shading = 0; shading <= 3; ++shading)
      for (int bits = 0; bits < 64; ++bits) {
        LaunchFacts f = small();
        f.isosurfaces = iso; f.shading = shading;
        f.translucent = bits & 1; f.ambient_occlusion = bits & 2; f.ranges = bits & 4; f.skipping = bits & 4; f.clip_on = bits & 8; f.orthographic = bits & 16; f.projection = (bits & 32) ? 2 : 0;
        f.isosurface_context = true;
        const LaunchPlan p = plan_launch(f);
        const int sh = shading <= 1 ? shading : 2;
        CHECK(!p.error && p.isosurface.on && p.isosurface.context && p.isosurface.translucent && p.isosurface.clipped, "isovalues %d shading %d bits %d: the clipped translucent plan with the flag", iso, shading, bits);
        CHECK(!p.isosurface.skip && !p.skip && !p.ambient_occlusion, "isovalues %d shading %d bits %d: neither skip nor the AO twins", iso, shading, bits);
        CHECK(p.shading == sh && p.orthographic == ((bits & 16) != 0) && p.am == 0, "isovalues %d shading %d bits %d: shading %d", iso, shading, bits, p.shading);
        CHECK(p.march_lds_bytes == 384 + 5152 && p.isosurface.lds_bytes == 384 + 5152, "lds %zu", p.march_lds_bytes);
        CHECK(plan_variants_exist(p, true) && isosurface_variant_exists(p.shading, p.am, false, true, p.orthographic, true, false, true), "the variant exists");
        CHECK(!p.pooled && p.project.mode == 0 && !p.slices.on && p.shade_grid_blocks == 0 && !p.cached, "nothing else of the plan is set");
        // against the translucent plan of the same facts without ranges and AO: the flag and the LDS size alone differ
        LaunchFacts g = f;
        g.isosurface_context = false; g.translucent = true; g.ambient_occlusion = false; g.ranges = false;
        LaunchPlan t = plan_launch(g);
        CHECK(t.isosurface.translucent && !t.isosurface.context && t.march_lds_bytes == 384, "the translucent plan: lds %zu", t.march_lds_bytes);
        t.isosurface.context = true; t.march_lds_bytes = t.isosurface.lds_bytes = 384 + 5152;
        CHECK(same_plan(p, t), "isovalues %d shading %d bits %d: the translucent plan plus the flag and the table", iso, shading, bits);
        ++n;
      }
  CHECK(n == 4 * 4 * 64, "%d plans", n);
  // the addressing modes: the tables in front of the transfer function (16-byte aligned), none in mode 3; the row loads on the 16-bit layouts
  LaunchFacts f = small();
  f.isosurfaces = 2; f.isosurface_context = true;
  for (int k = 0; k <= 3; ++k) {
    const LaunchPlan p = plan_launch(f, ov(k));
    CHECK(p.am == k && p.march_lds_bytes == 5152u + (k == 3 ? 0u : k == 2 ? 464u : 384u), "addressing %d: am %d lds %zu", k, p.am, p.march_lds_bytes);
  }
  LaunchFacts h = small(2);
  h.isosurfaces = 1; h.isosurface_context = true; h.row_loads = 2;
  LaunchPlan p = plan_launch(h);
  CHECK(p.am == 4 && p.isosurface.context && plan_variants_exist(p, false), "row loads: am %d", p.am);
  // errors: an oversized table (tf_lds_bytes gives 0 above 96 KiB), as the march has it; the isosurface frame of the same facts does not stage the table
  f = small(); f.isosurfaces = 2; f.isosurface_context = true; f.n_color = 8192;
  CHECK(plan_launch(f).error && !plan_launch(f).isosurface.on, "an oversized table");
  f.isosurface_context = false;
  CHECK(!plan_launch(f).error, "the isosurface frame does not stage it");
  f.isosurface_context = true; f.n_color = 256; f.isosurfaces = 5;
  CHECK(plan_launch(f).error, "five isovalues");
  f.isosurfaces = 1; f.quad = true;
  CHECK(plan_launch(f).error, "a quad layout");
  // the predicate: a translucent kernel on the clipped test alone, no skipping or AO twin, both cameras, three shading modes
  CHECK(isosurface_variant_exists(0, 0, false, true, false, true, false, true) && isosurface_variant_exists(2, 3, false, true, true, true, false, true)
          && !isosurface_variant_exists(2, 0, false, false, false, true, false, true) && !isosurface_variant_exists(2, 0, true, true, false, true, false, true)
          && !isosurface_variant_exists(2, 0, false, true, false, true, true, true) && !isosurface_variant_exists(2, 0, false, true, false, false, false, true)
          && !isosurface_variant_exists(3, 0, false, true, false, true, false, true) && !isosurface_variant_exists(0, 5, false, true, false, true, false, true),
        "the predicate");
}

// slices over the context; the mode kept at n = 0: without isovalues the fact is not read
static void precedence()
{
  int n = 0;
  for (int projection = 0; projection <= 3; ++projection)
    for (int shading = 0; shading <= 2; ++shading)
      for (int bits = 0; bits < 64; ++bits) {
        LaunchFacts f = small();
        f.projection = projection; f.shading = shading;
        f.pool = bits & 1; f.skipping = bits & 2; f.lds_staging = bits & 4; f.translucent = bits & 8; f.ambient_occlusion = bits & 16; f.shadow_cache = bits & 32;
        f.isosurfaces = 2; f.isosurface_context = true;
        // slices committed: the slice frame, as without the context fact
        LaunchFacts s = f;
        s.slices = 2; s.slice_walks = true; s.slice_extremum = true; s.ranges = true;
        LaunchFacts s_off = s;
        s_off.isosurface_context = false;
        const LaunchPlan a = plan_launch(s), b = plan_launch(s_off);
        CHECK(a.slices.on && !a.isosurface.on && !a.isosurface.context && same_plan(a, b), "slices over the context: projection %d shading %d bits %d", projection, shading, bits);
        // and under the slice context too
        s.slice_context = s_off.slice_context = true;
        CHECK(same_plan(plan_launch(s), plan_launch(s_off)) && plan_launch(s).slices.context && !plan_launch(s).isosurface.context, "slice context over the isosurface context");
        // no isovalue committed: the fact is kept and not read - the projection or march frame it was
        LaunchFacts z = f;
        z.isosurfaces = 0; z.translucent = false; z.ambient_occlusion = false;
        LaunchFacts z_off = z;
        z_off.isosurface_context = false;
        const LaunchPlan c = plan_launch(z), d = plan_launch(z_off);
        CHECK(!c.isosurface.on && !c.isosurface.context && same_plan(c, d) && c.project.mode == projection, "n = 0: projection %d shading %d bits %d", projection, shading, bits);
        ++n;
      }
  CHECK(n == 4 * 3 * 64, "%d plans", n);
}

// the fact false: every isosurface plan is the one section 17 / 19 / 20 state - literals - and no plan carries the flag
static void off_changes_nothing()
{
  int n = 0;
  for (int iso = 0; iso <= 4; ++iso)
    for (int projection = 0; projection <= 3; ++projection)
      for (int shading = 0; shading <= 2; ++shading)
        for (int bits = 0; bits < 256; ++bits)
          for (int k = -1; k <= 3; ++k) {
            LaunchFacts f = small(bits & 64 ? 2 : 4);
            f.shading = shading; f.projection = projection; f.isosurfaces = iso;
            f.pool = bits & 1; f.skipping = bits & 2; f.ranges = bits & 2; f.sparse = bits & 4; f.clip_on = bits & 8; f.translucent = iso > 0 && (bits & 16);
            f.ambient_occlusion = iso > 0 && (bits & 32); f.orthographic = bits & 128;
            const LaunchPlan a = plan_launch(f, ov(k));
            CHECK(!a.isosurface.context, "isovalues %d projection %d shading %d bits %d override %d: the flag without the fact", iso, projection, shading, bits, k);
            if (iso > 0) {
              // the isosurface frame's plan: the tables alone in LDS, skip by the ranges, the AO twins under a shading mode with an ambient term, translucent by
              // opacities or AO, clipped by box, camera or translucency
              const bool ao = (bits & 32) && shading >= 1, trans = (bits & 16) || ao;
              const int am = a.am;
              const size_t tables = am == 3 ? 0 : am == 2 ? (size_t)20 * 8 + 76 * 4 : (size_t)96 * 4;
              CHECK(!a.error && a.isosurface.on && a.shading == shading && a.isosurface.skip == ((bits & 2) != 0) && a.ambient_occlusion == ao && a.isosurface.translucent == trans
                      && a.isosurface.clipped == ((bits & 8) || (bits & 128) || trans) && a.march_lds_bytes == std::max<size_t>(tables, 128) && a.isosurface.lds_bytes == a.march_lds_bytes
                      && !a.slices.on && a.project.mode == 0 && !a.pooled,
                    "isovalues %d shading %d bits %d override %d: lds %zu", iso, shading, bits, k, a.march_lds_bytes);
            }
            ++n;
          }
  CHECK(n == 5 * 4 * 3 * 256 * 5, "%d plans", n);
  // the trailing default of the predicate: the seven-argument calls read as before
  CHECK(isosurface_variant_exists(2, 0, true, false) && !isosurface_variant_exists(2, 0, true, false, true) && isosurface_variant_exists(1, 0, true, true, true, true, true)
          && !isosurface_variant_exists(0, 0, false, true, false, true, true),
        "the predicate without the context");
}

// ovr_hip_set_isosurface_context is recorded under kShading, like the other frame kinds: the accumulation starts over, nothing else is voided
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
