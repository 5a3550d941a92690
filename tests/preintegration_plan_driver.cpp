// Driver of tests/test_preintegration_plan.py: the pre-integrated march's part of csrc/host/launch_plan.hpp, its known-answer row of csrc/host/ray_query.hpp and the
// commit plan's row of the frame kinds on the CPU.  `driver <scenario>` exits 0 when every row of the scenario's table gave what the row expects; the
// expectations are literals, worked out by hand per row.
#include "commit_plan.hpp"
#include "launch_plan.hpp"
#include "plan_compare.hpp"
#include "ray_query.hpp"

#include <cstdio>
#include <cstring>
#include <string>

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
static bool same_preintegrated(const LaunchPlan& a, const LaunchPlan& b)
{
  return a.preintegrated.on == b.preintegrated.on && a.preintegrated.clipped == b.preintegrated.clipped && a.preintegrated.lds_bytes == b.preintegrated.lds_bytes
         && a.preintegrated.subdivision == b.preintegrated.subdivision && a.preintegrated.nodes == b.preintegrated.nodes;
}

// the kind, the clipped kernel for both cameras, LDS = tables + transfer function + node table, no skipping, no pool, no LDS staging
static void preintegrated()
{
  // tables 4 * (40 + 33 + 3 + 18 + 2) = 384 bytes; the transfer function 256 * 16 + 256 * 4 + 32 = 5152; S = 4: M = 1021, 16 * 1022 = 16352
  for (int bits = 0; bits < 128; ++bits) {
    LaunchFacts f = small();
    f.preintegrated = true;
    f.clip_on = bits & 1; f.orthographic = bits & 2; f.skipping = bits & 4; f.ranges = bits & 4; f.lds_staging = bits & 8; f.pool = bits & 16; f.sparse = bits & 32; f.shadow_cache = bits & 64;
    const LaunchPlan p = plan_launch(f);
    CHECK(!p.error && p.preintegrated.on && frame_kind(p) == FrameKind::PreintegratedMarch, "bits %d: the kind", bits);
    CHECK(p.preintegrated.clipped && p.orthographic == ((bits & 2) != 0), "bits %d: the clipped kernel with the unit box, the camera's twin", bits);
    CHECK(!p.skip && !p.pooled && !p.march.lds_staged && !p.march.deep && !p.cached && p.shading == 0 && p.shade_grid_blocks == 0, "bits %d: it fetches every step, in place", bits);
    CHECK(p.preintegrated.subdivision == 4 && p.preintegrated.nodes == 1021, "bits %d: S %d M %d", bits, p.preintegrated.subdivision, p.preintegrated.nodes);
    CHECK(p.march_lds_bytes == 384 + 5152 + 16352 && p.preintegrated.lds_bytes == p.march_lds_bytes, "bits %d: lds %zu", bits, p.march_lds_bytes);
    CHECK(plan_variants_exist(p, true) && preintegrated_variant_exists(p.am, p.skip, p.preintegrated.clipped, p.orthographic), "bits %d: the variant exists", bits);
    CHECK(p.project.mode == 0 && !p.isosurface.on && !p.slices.on && !p.ambient_occlusion, "bits %d: nothing else of the plan is set", bits);
  }
  // the addressing modes: the tables in front of the transfer function (16-byte aligned), none in mode 3; the row loads on the 16-bit layouts
  LaunchFacts f = small();
  f.preintegrated = true;
  for (int k = 0; k <= 3; ++k) {
    const LaunchPlan p = plan_launch(f, ov(k));
    CHECK(p.am == k && p.march_lds_bytes == 5152u + 16352u + (k == 3 ? 0u : k == 2 ? 464u : 384u), "addressing %d: am %d lds %zu", k, p.am, p.march_lds_bytes);
  }
  LaunchFacts h = small(2);
  h.preintegrated = true; h.row_loads = 2;
  LaunchPlan p = plan_launch(h);
  CHECK(p.am == 4 && p.preintegrated.on && plan_variants_exist(p, false), "row loads: am %d", p.am);
  // unequal tables: the finer one counts; a one-entry pair has one segment.  The node table starts 16-byte aligned behind a transfer function of any size
  f = small(); f.preintegrated = true; f.n_color = 16; f.n_alpha = 64;
  p = plan_launch(f);
  CHECK(p.preintegrated.nodes == 253 && p.march_lds_bytes == 384 + 544 + 16 * 254, "16 colours, 64 alphas: M %d lds %zu", p.preintegrated.nodes, p.march_lds_bytes);
  f.n_color = 3; f.n_alpha = 3; // 48 + 12 + 32 = 92 bytes: the node table starts at 384 + 96
  p = plan_launch(f);
  CHECK(p.preintegrated.nodes == 9 && p.march_lds_bytes == 384 + 96 + 160, "3 / 3: M %d lds %zu", p.preintegrated.nodes, p.march_lds_bytes);
  f.nx = f.ny = f.nz = 1; f.n_color = f.n_alpha = 1;
  p = plan_launch(f, ov(3));
  CHECK(!p.error && p.preintegrated.nodes == 5 && p.march_lds_bytes == 64 + 96, "mode 3, one-entry tables (52 bytes, aligned 64): lds %zu", p.march_lds_bytes);
  // the predicate: clipped alone, no skipping twin, both cameras
  CHECK(preintegrated_variant_exists(0, false, true) && preintegrated_variant_exists(3, false, true, true) && preintegrated_variant_exists(4, false, true) && !preintegrated_variant_exists(0, false, false)
          && !preintegrated_variant_exists(0, true, true) && !preintegrated_variant_exists(5, false, true) && !preintegrated_variant_exists(-1, false, true),
        "the predicate");
}

// the LDS budget: 54608 bytes = a third of 160 KiB, a multiple of 16.  S gives way first, then the frame is an error
static void budget()
{
  CHECK(kPreintegrationLdsBudget == 54608, "the budget: %zu", kPreintegrationLdsBudget);
  struct Row { int nc, na, s, m; bool error; };
  // tables 384.  nc = na = n: the transfer function takes 20 n + 32, the node table 16 * (S (n - 1) + 2)
  //   n = 256: 5152; S = 4: 16352 -> 21888 fits
  //   n = 700: 14032, front 14416; room 40192: S = 4 needs 16 * 2798 = 44768 (no), S = 2 16 * 1400 = 22400 fits
  //   n = 1200: 24032, front 24416; room 30192: S = 2 needs 16 * 2400 = 38400 (no), S = 1 16 * 1201 = 19216 fits
  //   n = 1600: 32032, front 32416; room 22192: S = 1 needs 16 * 1601 = 25616: an error
  const Row rows[] = { { 256, 256, 4, 1021, false }, { 700, 700, 2, 1399, false }, { 1200, 1200, 1, 1200, false }, { 1600, 1600, 0, 0, true },
                       { 16, 3000, 0, 0, true } /* 256 + 12000 + 32 = 12288, front 12672; room 41936: S = 1 needs 16 * 3001 = 48016 */,
                       { 16, 2500, 1, 2500, false } /* 10288, front 10672; room 43936 >= 16 * 2501 = 40016 */ };
  for (const Row& r : rows) {
    LaunchFacts f = small();
    f.preintegrated = true; f.n_color = r.nc; f.n_alpha = r.na;
    const LaunchPlan p = plan_launch(f);
    CHECK(p.error == r.error && p.preintegrated.on == !r.error && p.preintegrated.subdivision == r.s && p.preintegrated.nodes == r.m, "%d / %d: error %d S %d M %d", r.nc, r.na, (int)p.error,
          p.preintegrated.subdivision, p.preintegrated.nodes);
    CHECK(p.error || p.march_lds_bytes <= kPreintegrationLdsBudget, "%d / %d: lds %zu", r.nc, r.na, p.march_lds_bytes);
    if (r.error) { // the march of the same facts still runs: the mode costs nothing until it is drawn
      f.preintegrated = false;
      CHECK(!plan_launch(f).error, "%d / %d: the march", r.nc, r.na);
    }
  }
  // a transfer function too large for its own staging is the march's error too
  LaunchFacts f = small();
  f.preintegrated = true; f.n_color = 8192;
  CHECK(plan_launch(f).error && !plan_launch(f).preintegrated.on, "an oversized table");
  f = small(); f.preintegrated = true; f.quad = true;
  CHECK(plan_launch(f).error, "a quad layout");
  f = small(); f.preintegrated = true; f.tables = false;
  CHECK(plan_launch(f).error && !plan_launch(f, ov(3)).error, "no axis tables: mode 3 alone");
}

// taken exactly under March + shading 0; with the fact false every plan is what the facts planned before the kind existed
static void off_changes_nothing()
{
  int n = 0, taken = 0;
  for (int slices = 0; slices <= 2; ++slices)
    for (int iso = 0; iso <= 2; ++iso)
      for (int projection = 0; projection <= 3; ++projection)
        for (int shading = 0; shading <= 2; ++shading)
          for (int bits = 0; bits < 512; ++bits)
            for (int k = -1; k <= 3; k += 2) {
              LaunchFacts f = small(bits & 64 ? 2 : 4);
              f.shading = shading; f.projection = projection; f.slices = slices; f.isosurfaces = iso;
              f.pool = bits & 1; f.skipping = bits & 2; f.sparse = bits & 4; f.clip_on = bits & 8; f.lds_staging = bits & 16; f.slice_context = bits & 32; f.isosurface_context = bits & 32;
              f.ranges = bits & 128; f.orthographic = bits & 256;
              const LaunchPlan off = plan_launch(f, ov(k));
              CHECK(!off.preintegrated.on && off.preintegrated.lds_bytes == 0 && off.preintegrated.nodes == 0 && frame_kind(off) != FrameKind::PreintegratedMarch,
                    "slices %d isovalues %d projection %d shading %d bits %d override %d: the kind without the fact", slices, iso, projection, shading, bits, k);
              f.preintegrated = true;
              const LaunchPlan on = plan_launch(f, ov(k));
              const bool march = slices == 0 && iso == 0 && projection == 0;
              if (march && shading == 0) {
                CHECK(on.preintegrated.on && frame_kind(on) == FrameKind::PreintegratedMarch && !on.error, "bits %d override %d: taken", bits, k);
                ++taken;
              }
              else // kept and not drawn: the plan of the facts without it, member for member
                CHECK(!on.preintegrated.on && same_plan(on, off) && same_preintegrated(on, off) && frame_kind(on) == frame_kind(off),
                      "slices %d isovalues %d projection %d shading %d bits %d override %d: kept, not drawn", slices, iso, projection, shading, bits, k);
              ++n;
            }
  CHECK(n == 3 * 3 * 4 * 3 * 512 * 3 && taken == 512 * 3, "%d plans, %d taken", n, taken);
  // the literals of tests/slice_context_plan_driver.cpp, again: the unshaded march 5152 + 384, one plane 384
  LaunchFacts f = small();
  LaunchPlan p = plan_launch(f);
  CHECK(!p.error && frame_kind(p) == FrameKind::March && p.march_lds_bytes == 5152 + 384, "unshaded march: lds %zu", p.march_lds_bytes);
  f.slices = 1; f.preintegrated = true;
  p = plan_launch(f);
  CHECK(!p.error && p.slices.on && !p.preintegrated.on && p.march_lds_bytes == 384, "one plane under SEGMENTS: lds %zu", p.march_lds_bytes);
  // the new kind stands behind the nine the other drivers loop over
  CHECK((int)FrameKind::PreintegratedMarch == (int)FrameKind::SliceContext + 1 && (int)FrameKind::March == 0, "appended after SliceContext");
}

// the known-answer row: outside the table of seven, its refusals in order, its record
static void query_row()
{
  CHECK(kRayQueryCount == 7 && sizeof(kRayQueries) / sizeof(kRayQueries[0]) == 7 && kQueryPreintegrated == 7 && kRayQueryIds == 8, "the table keeps its seven rows");
  const RayQuery& d = ray_query_row(kQueryPreintegrated);
  CHECK(&d == &kPreintegrationQueries[0] && &ray_query_row(kQuerySliceContext) == &kRayQueries[kQuerySliceContext], "the lookup");
  CHECK(!strcmp(d.name, "ovr_hip_preintegrated_floats") && d.kind == FrameKind::PreintegratedMarch && d.needs == QueryNeeds::Nothing && d.needs_preintegration && d.needs_tf && !d.needs_context
          && !d.needs_ao && !d.takes_range_skipping && !d.takes_max_events && !d.takes_rotation && !d.takes_mode && !d.zeroed,
        "the row");
  for (int k = 0; k < kRayQueryCount; ++k) CHECK(!kRayQueries[k].needs_preintegration, "row %d: the trailing member's default", k);
  CHECK(ray_query_record_floats(d, 0) == 8 && ray_query_record_floats(d, 16) == 8, "8 floats per ray");
  CHECK(query_runs(d, FrameKind::PreintegratedMarch) && !query_runs(d, FrameKind::March) && !query_runs(d, FrameKind::SliceContext), "its own kind alone");
  // refusals: volume, pre-integration, transfer function - in this order
  QueryFacts f;
  QueryStatus s = ray_query_preconditions(d, f, false);
  CHECK(s.code == -3 && s.message == "[hip] ovr_hip_preintegrated_floats: no volume was set", "%d %s", s.code, s.message.c_str());
  f.volume = true;
  s = ray_query_preconditions(d, f, false);
  CHECK(s.code == -3 && s.message == "[hip] ovr_hip_preintegrated_floats: no pre-integration is committed (ovr_hip_set_preintegration)", "%d %s", s.code, s.message.c_str());
  f.transfer_function = true; // (without the mode the message is still the mode's)
  s = ray_query_preconditions(d, f, false);
  CHECK(s.code == -3 && s.message == "[hip] ovr_hip_preintegrated_floats: no pre-integration is committed (ovr_hip_set_preintegration)", "%d %s", s.code, s.message.c_str());
  f.transfer_function = false; f.preintegration = true;
  s = ray_query_preconditions(d, f, false);
  CHECK(s.code == -3 && s.message == "[hip] ovr_hip_preintegrated_floats: no transfer function was committed", "%d %s", s.code, s.message.c_str());
  f.transfer_function = true;
  CHECK(ray_query_preconditions(d, f, false).code == 0 && ray_query_preconditions(d, f, true).code == 0, "granted, whatever slices and isovalues are committed");
  f.slices = 2; f.isovalues = 3;
  CHECK(ray_query_preconditions(d, f, false).code == 0, "granted under committed slices");
  // the other entries do not ask for the mode
  QueryFacts g;
  g.volume = true;
  CHECK(ray_query_preconditions(kRayQueries[kQueryProject], g, false).code == 0, "ovr_hip_project_floats without the mode");
  // arguments
  RayQueryCall c;
  const float x = 0.f;
  float y = 0.f;
  s = ray_query_arguments(d, true, c);
  CHECK(s.code == -1 && s.message == "[hip] ovr_hip_preintegrated_floats: bad arguments", "%d %s", s.code, s.message.c_str());
  c.org = &x; c.dir = &x; c.out = &y; c.n = 0;
  CHECK(ray_query_arguments(d, true, c).code == 0 && ray_query_arguments(d, false, c).code == -1, "pointers and a renderer");
  c.n = -1;
  CHECK(ray_query_arguments(d, true, c).code == -1, "n < 0");
}

// ovr_hip_set_preintegration is recorded under kShading, like the other frame kinds: the accumulation starts over, nothing else is voided
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
  Changes same; // the same mode again: still a call
  same.note(kShading, true, false);
  CHECK(plan_commit(same, facts).what == kChanged, "the same value again");
  Changes none;
  CHECK(plan_commit(none, facts).what == 0u, "no call, no effect");
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "preintegrated", preintegrated }, { "budget", budget }, { "off_changes_nothing", off_changes_nothing }, { "query_row", query_row }, { "commit_row", commit_row } };

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
