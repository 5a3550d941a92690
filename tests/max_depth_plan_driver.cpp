// Driver of tests/test_max_depth_plan.py: the depth-limited march's part of csrc/host/launch_plan.hpp, its known-answer row of csrc/host/ray_query.hpp and the
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
static bool same_kinds(const LaunchPlan& a, const LaunchPlan& b)
{
  return a.max_depth.on == b.max_depth.on && a.max_depth.clipped == b.max_depth.clipped && a.max_depth.shade == b.max_depth.shade && a.max_depth.lds_bytes == b.max_depth.lds_bytes
         && a.gradient_opacity.on == b.gradient_opacity.on && a.gradient_opacity.shade == b.gradient_opacity.shade && a.gradient_opacity.lds_bytes == b.gradient_opacity.lds_bytes
         && a.preintegrated.on == b.preintegrated.on && a.preintegrated.nodes == b.preintegrated.nodes && a.preintegrated.lds_bytes == b.preintegrated.lds_bytes;
}

// the kind, the clipped kernel for both cameras and both shading modes, LDS = tables + transfer function, no skipping, no pool, no LDS staging
static void variants()
{
  // tables 4 * (40 + 33 + 3 + 18 + 2) = 384 bytes; the transfer function 256 * 16 + 256 * 4 + 32 = 5152
  for (int shading = 0; shading <= 1; ++shading)
    for (int bits = 0; bits < 128; ++bits) {
      LaunchFacts f = small();
      f.max_depth = true; f.shading = shading;
      f.clip_on = bits & 1; f.orthographic = bits & 2; f.skipping = bits & 4; f.ranges = bits & 4; f.lds_staging = bits & 8; f.pool = bits & 16; f.sparse = bits & 32; f.shadow_cache = bits & 64;
      const LaunchPlan p = plan_launch(f);
      CHECK(!p.error && p.max_depth.on && frame_kind(p) == FrameKind::DepthLimitedMarch, "shading %d bits %d: the kind", shading, bits);
      CHECK(p.max_depth.clipped && p.orthographic == ((bits & 2) != 0) && p.max_depth.shade == (shading == 1), "shading %d bits %d: the clipped kernel with the unit box, the camera's and the shading's twin", shading, bits);
      CHECK(!p.skip && !p.pooled && !p.march.lds_staged && !p.march.deep && !p.cached && p.shading == shading && p.shade_grid_blocks == 0, "shading %d bits %d: it fetches every step, in place", shading, bits);
      CHECK(p.march_lds_bytes == 384 + 5152 && p.max_depth.lds_bytes == p.march_lds_bytes, "shading %d bits %d: lds %zu", shading, bits, p.march_lds_bytes);
      CHECK(plan_variants_exist(p, true) && max_depth_variant_exists(shading, p.am, p.skip, p.max_depth.clipped, p.orthographic), "shading %d bits %d: the variant exists", shading, bits);
      CHECK(p.project.mode == 0 && !p.isosurface.on && !p.slices.on && !p.preintegrated.on && !p.gradient_opacity.on && !p.ambient_occlusion, "shading %d bits %d: nothing else of the plan is set", shading, bits);
    }
  // the addressing modes: the tables in front of the transfer function (16-byte aligned), none in mode 3; the row loads on the 16-bit layouts
  LaunchFacts f = small();
  f.max_depth = true;
  for (int k = 0; k <= 3; ++k) {
    const LaunchPlan p = plan_launch(f, ov(k));
    CHECK(p.am == k && p.march_lds_bytes == 5152u + (k == 3 ? 0u : k == 2 ? 464u : 384u), "addressing %d: am %d lds %zu", k, p.am, p.march_lds_bytes);
  }
  LaunchFacts h = small(2);
  h.max_depth = true; h.row_loads = 2; h.shading = 1;
  LaunchPlan p = plan_launch(h);
  CHECK(p.am == 4 && p.max_depth.on && p.max_depth.shade && plan_variants_exist(p, false), "row loads: am %d", p.am);
  // a tiny volume in mode 3 under one-entry tables: the counter reduction's words are the floor
  f.nx = f.ny = f.nz = 1; f.n_color = f.n_alpha = 1;
  p = plan_launch(f, ov(3));
  CHECK(!p.error && p.march_lds_bytes == (size_t)kWaves * kCounterWords * 4 && p.march_lds_bytes >= 52, "mode 3, one-entry tables: lds %zu", p.march_lds_bytes);
  // errors: a transfer function too large for its own staging, a quad layout, no axis tables below mode 3
  f = small(); f.max_depth = true; f.n_color = 8192;
  CHECK(plan_launch(f).error && !plan_launch(f).max_depth.on, "an oversized table");
  f = small(); f.max_depth = true; f.quad = true;
  CHECK(plan_launch(f).error, "a quad layout");
  f = small(); f.max_depth = true; f.tables = false;
  CHECK(plan_launch(f).error && !plan_launch(f, ov(3)).error, "no axis tables: mode 3 alone");
  // the predicate: shading NONE and GRADIENT, clipped alone, no skipping twin, both cameras
  CHECK(max_depth_variant_exists(0, 0, false, true) && max_depth_variant_exists(1, 3, false, true, true) && max_depth_variant_exists(1, 4, false, true)
          && !max_depth_variant_exists(2, 0, false, true) && !max_depth_variant_exists(-1, 0, false, true) && !max_depth_variant_exists(0, 0, false, false)
          && !max_depth_variant_exists(0, 0, true, true) && !max_depth_variant_exists(1, 5, false, true) && !max_depth_variant_exists(0, -1, false, true),
        "the predicate");
}

// taken exactly under March + shading 0 or 1 + no active pre-integration + no active gradient opacity; with the fact false every plan is what the facts planned
// before the kind existed
static void precedence()
{
  int n = 0, taken = 0;
  for (int slices = 0; slices <= 2; ++slices)
    for (int iso = 0; iso <= 2; ++iso)
      for (int projection = 0; projection <= 3; ++projection)
        for (int shading = 0; shading <= 2; ++shading)
          for (int pre = 0; pre <= 1; ++pre)
            for (int gradop = 0; gradop <= 1; ++gradop)
              for (int bits = 0; bits < 512; ++bits)
                for (int k = -1; k <= 3; k += 2) {
                  LaunchFacts f = small(bits & 64 ? 2 : 4);
                  f.shading = shading; f.projection = projection; f.slices = slices; f.isosurfaces = iso; f.preintegrated = pre != 0; f.gradient_opacity = gradop != 0;
                  f.pool = bits & 1; f.skipping = bits & 2; f.sparse = bits & 4; f.clip_on = bits & 8; f.lds_staging = bits & 16; f.slice_context = bits & 32; f.isosurface_context = bits & 32;
                  f.ranges = bits & 128; f.orthographic = bits & 256;
                  const LaunchPlan off = plan_launch(f, ov(k));
                  CHECK(!off.max_depth.on && off.max_depth.lds_bytes == 0 && frame_kind(off) != FrameKind::DepthLimitedMarch,
                        "slices %d isovalues %d projection %d shading %d pre %d gradop %d bits %d override %d: the kind without the fact", slices, iso, projection, shading, pre, gradop, bits, k);
                  f.max_depth = true;
                  const LaunchPlan on = plan_launch(f, ov(k));
                  const bool march = slices == 0 && iso == 0 && projection == 0;
                  const bool preintegrated = march && shading == 0 && pre != 0; // pre-integration's own rule
                  const bool gradient_opacity = gradient_opacity_active(gradop, march, shading, preintegrated); // gradient opacity's own rule
                  if (march && shading <= 1 && !preintegrated && !gradient_opacity) {
                    CHECK(on.max_depth.on && frame_kind(on) == FrameKind::DepthLimitedMarch && !on.error && on.max_depth.shade == (shading == 1), "shading %d bits %d override %d: taken", shading, bits, k);
                    ++taken;
                  }
                  else // kept and not drawn: the plan of the facts without it, member for member
                    CHECK(!on.max_depth.on && same_plan(on, off) && same_kinds(on, off) && frame_kind(on) == frame_kind(off),
                          "slices %d isovalues %d projection %d shading %d pre %d gradop %d bits %d override %d: kept, not drawn", slices, iso, projection, shading, pre, gradop, bits, k);
                  CHECK(max_depth_active(true, march, shading, preintegrated, gradient_opacity, true) == on.max_depth.on, "the host header's rule is the plan's");
                  ++n;
                }
  CHECK(n == 3 * 3 * 4 * 3 * 2 * 2 * 512 * 3 && taken == 3 * 512 * 3, "%d plans, %d taken", n, taken); // (without gradient opacity alone: shading 0 without, shading 1 with and without pre-integration)
  // the literals of tests/slice_context_plan_driver.cpp, again: the unshaded march 5152 + 384, one plane 384
  LaunchFacts f = small();
  LaunchPlan p = plan_launch(f);
  CHECK(!p.error && frame_kind(p) == FrameKind::March && p.march_lds_bytes == 5152 + 384, "unshaded march: lds %zu", p.march_lds_bytes);
  f.slices = 1; f.max_depth = true;
  p = plan_launch(f);
  CHECK(!p.error && p.slices.on && !p.max_depth.on && p.march_lds_bytes == 384, "one plane under an image: lds %zu", p.march_lds_bytes);
  f = small(); f.max_depth = true; f.preintegrated = true;
  p = plan_launch(f);
  CHECK(!p.error && p.preintegrated.on && !p.max_depth.on && frame_kind(p) == FrameKind::PreintegratedMarch, "pre-integration under shading NONE goes first");
  f = small(); f.max_depth = true; f.gradient_opacity = true; f.shading = 1;
  p = plan_launch(f);
  CHECK(!p.error && p.gradient_opacity.on && !p.max_depth.on && frame_kind(p) == FrameKind::GradientOpacityMarch, "gradient opacity goes first");
  f = small(); f.max_depth = true; f.shading = 2;
  p = plan_launch(f);
  CHECK(!p.error && !p.max_depth.on && frame_kind(p) == FrameKind::March && p.shading == 2, "FULL shading: kept, not drawn");
  // the new kind stands behind the eleven the other drivers loop over
  CHECK((int)FrameKind::DepthLimitedMarch == (int)FrameKind::GradientOpacityMarch + 1 && (int)FrameKind::GradientOpacityMarch == (int)FrameKind::PreintegratedMarch + 1 && (int)FrameKind::March == 0,
        "appended last");
}

// the known-answer row: outside the table of seven and behind the gradient opacity's, its refusals in order, its record
static void query_row()
{
  CHECK(kRayQueryCount == 7 && sizeof(kRayQueries) / sizeof(kRayQueries[0]) == 7 && kQueryPreintegrated == 7 && kRayQueryIds == 8 && kQueryGradientOpacity == 8 && kRayQueryRows == 9
          && kQueryMaxDepth == 9 && kRayQueryAll == 10,
        "the table keeps its seven rows, the two rows behind it their ids");
  const RayQuery& d = ray_query_row(kQueryMaxDepth);
  CHECK(&d == &kMaxDepthQueries[0] && &ray_query_row(kQueryGradientOpacity) == &kGradientOpacityQueries[0] && &ray_query_row(kQueryPreintegrated) == &kPreintegrationQueries[0]
          && &ray_query_row(kQuerySliceContext) == &kRayQueries[kQuerySliceContext],
        "the lookup");
  CHECK(!strcmp(d.name, "ovr_hip_max_depth_floats") && d.kind == FrameKind::DepthLimitedMarch && d.needs == QueryNeeds::Nothing && d.takes_depth && d.takes_shade && d.needs_tf
          && !d.needs_gradient_opacity && !d.needs_preintegration && !d.needs_context && !d.needs_ao && !d.takes_range_skipping && !d.takes_max_events && !d.takes_rotation && !d.takes_mode && !d.zeroed,
        "the row");
  for (int k = 0; k < kRayQueryRows; ++k) CHECK(!ray_query_row(k).takes_depth, "row %d: the trailing member's default", k);
  CHECK(ray_query_record_floats(d, 0) == 8 && ray_query_record_floats(d, 16) == 8, "8 floats per ray");
  CHECK(query_runs(d, FrameKind::DepthLimitedMarch) && !query_runs(d, FrameKind::March) && !query_runs(d, FrameKind::GradientOpacityMarch), "its own kind alone");
  // refusals: volume, transfer function - nothing else needs to be committed: the depths are the caller's
  QueryFacts f;
  QueryStatus s = ray_query_preconditions(d, f, false);
  CHECK(s.code == -3 && s.message == "[hip] ovr_hip_max_depth_floats: no volume was set", "%d %s", s.code, s.message.c_str());
  f.volume = true;
  s = ray_query_preconditions(d, f, false);
  CHECK(s.code == -3 && s.message == "[hip] ovr_hip_max_depth_floats: no transfer function was committed", "%d %s", s.code, s.message.c_str());
  f.transfer_function = true;
  CHECK(ray_query_preconditions(d, f, false).code == 0 && ray_query_preconditions(d, f, true).code == 0, "granted");
  f.slices = 2; f.isovalues = 3; f.preintegration = true; f.gradient_opacity = true;
  CHECK(ray_query_preconditions(d, f, false).code == 0, "granted under committed slices, isovalues, pre-integration and gradient opacity");
  // arguments: a depth per ray; the shading mode is NONE or GRADIENT
  RayQueryCall c;
  const float x = 0.f;
  float y = 0.f;
  s = ray_query_arguments(d, true, c);
  CHECK(s.code == -1 && s.message == "[hip] ovr_hip_max_depth_floats: bad arguments", "%d %s", s.code, s.message.c_str());
  c.org = &x; c.dir = &x; c.out = &y; c.n = 0;
  CHECK(ray_query_arguments(d, true, c).code == -1, "no depths");
  c.depth = &x;
  CHECK(ray_query_arguments(d, true, c).code == 0 && ray_query_arguments(d, false, c).code == -1, "pointers and a renderer");
  c.mode = 1;
  CHECK(ray_query_arguments(d, true, c).code == 0, "shade 1");
  c.mode = 2;
  CHECK(ray_query_arguments(d, true, c).code == -1, "shade 2");
  c.mode = -1;
  CHECK(ray_query_arguments(d, true, c).code == -1, "shade -1");
  c.mode = 0; c.n = -1;
  CHECK(ray_query_arguments(d, true, c).code == -1, "n < 0");
  // the other entries do not ask for depths
  RayQueryCall g;
  g.org = &x; g.dir = &x; g.out = &y;
  CHECK(ray_query_arguments(ray_query_row(kQueryGradientOpacity), true, g).code == 0 && ray_query_arguments(kRayQueries[kQuerySliceContext], true, g).code == 0, "no depths elsewhere");
}

// ovr_hip_set_max_depth is recorded under kShading, like the other frame kinds: the accumulation starts over, nothing else is voided
static void commit_row()
{
  using namespace commit;
  Changes c;
  c.note(kShading, true, true); // every call with an image counts as a change: contents are not compared
  CommitFacts facts;
  facts.framebuffer = facts.volume = true;
  const Effects e = plan_commit(c, facts);
  CHECK(e.has(kReset) && e.what == kChanged, "the accumulation starts over and nothing else follows: %#x", e.what);
  CHECK(!e.has(kResort) && !e.has(kRelist) && !e.has(kMajorantVoid) && !e.has(kRangesVoid) && !e.has(kLatticeStale) && !e.has(kSkipRestart), "nothing is voided: %#x", e.what);
  Changes none;
  CHECK(plan_commit(none, facts).what == 0u, "no call, no effect");
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "variants", variants }, { "precedence", precedence }, { "query_row", query_row }, { "commit_row", commit_row } };

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
