// Driver of tests/test_depth_output_plan.py: the depth-output march's part of csrc/host/launch_plan.hpp, its known-answer row of csrc/host/ray_query.hpp and the
// commit plan's row of the frame kinds on the CPU.  `driver <scenario>` exits 0 when every row of the scenario's table gave what the row expects; the
// expectations are literals, worked out by hand per row.  `driver rule <on> <slices> <isovalues> <projection> <shading> <pre> <gradop> <max_depth>` prints the
// planned kind's number and the plan's `limited`, for the comparison with depth_output.active.
#include "commit_plan.hpp"
#include "launch_plan.hpp"
#include "plan_compare.hpp"
#include "ray_query.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
  return a.depth_output.on == b.depth_output.on && a.depth_output.limited == b.depth_output.limited && a.depth_output.lds_bytes == b.depth_output.lds_bytes
         && a.max_depth.on == b.max_depth.on && a.max_depth.clipped == b.max_depth.clipped && a.max_depth.shade == b.max_depth.shade && a.max_depth.lds_bytes == b.max_depth.lds_bytes
         && a.gradient_opacity.on == b.gradient_opacity.on && a.gradient_opacity.shade == b.gradient_opacity.shade && a.gradient_opacity.lds_bytes == b.gradient_opacity.lds_bytes
         && a.preintegrated.on == b.preintegrated.on && a.preintegrated.nodes == b.preintegrated.nodes && a.preintegrated.lds_bytes == b.preintegrated.lds_bytes;
}

// the kind, the clipped kernel for both cameras and both shading modes, LDS = tables + transfer function, no skipping, no pool, no LDS staging
static void variants()
{
  // tables 4 * (40 + 33 + 3 + 18 + 2) = 384 bytes; the transfer function 256 * 16 + 256 * 4 + 32 = 5152: the depth-limited march's carve
  for (int shading = 0; shading <= 1; ++shading)
    for (int limited = 0; limited <= 1; ++limited)
      for (int bits = 0; bits < 128; ++bits) {
        LaunchFacts f = small();
        f.depth_output = true; f.depth_threshold = 0.5f; f.max_depth = limited != 0; f.shading = shading;
        f.clip_on = bits & 1; f.orthographic = bits & 2; f.skipping = bits & 4; f.ranges = bits & 4; f.lds_staging = bits & 8; f.pool = bits & 16; f.sparse = bits & 32; f.shadow_cache = bits & 64;
        const LaunchPlan p = plan_launch(f);
        CHECK(!p.error && p.depth_output.on && !p.max_depth.on && frame_kind(p) == FrameKind::DepthOutputMarch, "shading %d bits %d: the kind", shading, bits);
        CHECK(p.depth_output.limited == (limited != 0), "shading %d bits %d: limited %d", shading, bits, limited);
        CHECK(p.depth_output.clipped && p.orthographic == ((bits & 2) != 0) && p.depth_output.shade == (shading == 1), "shading %d bits %d: the clipped kernel with the unit box, the camera's and the shading's twin", shading, bits);
        CHECK(!p.skip && !p.pooled && !p.march.lds_staged && !p.march.deep && !p.cached && p.shading == shading && p.shade_grid_blocks == 0, "shading %d bits %d: it fetches every step, in place", shading, bits);
        CHECK(p.march_lds_bytes == 384 + 5152 && p.depth_output.lds_bytes == p.march_lds_bytes, "shading %d bits %d: lds %zu", shading, bits, p.march_lds_bytes);
        CHECK(plan_variants_exist(p, true) && depth_output_variant_exists(shading, p.am, p.skip, p.depth_output.clipped, p.orthographic), "shading %d bits %d: the variant exists", shading, bits);
        CHECK(p.project.mode == 0 && !p.isosurface.on && !p.slices.on && !p.preintegrated.on && !p.gradient_opacity.on && !p.ambient_occlusion, "shading %d bits %d: nothing else of the plan is set", shading, bits);
      }
  LaunchFacts f = small();
  f.depth_output = true;
  for (int k = 0; k <= 3; ++k) {
    const LaunchPlan p = plan_launch(f, ov(k));
    CHECK(p.am == k && p.march_lds_bytes == 5152u + (k == 3 ? 0u : k == 2 ? 464u : 384u), "addressing %d: am %d lds %zu", k, p.am, p.march_lds_bytes);
  }
  LaunchFacts h = small(2);
  h.depth_output = true; h.row_loads = 2; h.shading = 1;
  LaunchPlan p = plan_launch(h);
  CHECK(p.am == 4 && p.depth_output.on && p.depth_output.shade && plan_variants_exist(p, false), "row loads: am %d", p.am);
  f.nx = f.ny = f.nz = 1; f.n_color = f.n_alpha = 1;
  p = plan_launch(f, ov(3));
  CHECK(!p.error && p.march_lds_bytes == (size_t)kWaves * kCounterWords * 4 && p.march_lds_bytes >= 52, "mode 3, one-entry tables: lds %zu", p.march_lds_bytes);
  f = small(); f.depth_output = true; f.n_color = 8192;
  CHECK(plan_launch(f).error && !plan_launch(f).depth_output.on, "an oversized table");
  f = small(); f.depth_output = true; f.quad = true;
  CHECK(plan_launch(f).error, "a quad layout");
  f = small(); f.depth_output = true; f.tables = false;
  CHECK(plan_launch(f).error && !plan_launch(f, ov(3)).error, "no axis tables: mode 3 alone");
  // the predicate is the depth-limited kernel's
  for (int shade = -1; shade <= 2; ++shade)
    for (int am = -1; am <= 5; ++am)
      for (int bits = 0; bits < 8; ++bits)
        CHECK(depth_output_variant_exists(shade, am, bits & 1, bits & 2, bits & 4) == max_depth_variant_exists(shade, am, bits & 1, bits & 2, bits & 4), "shade %d am %d bits %d", shade, am, bits);
}

// taken exactly under March + shading 0 or 1 + no active pre-integration + no active gradient opacity, whether or not a depth image is bound; with the fact
// false every plan is what the facts planned before the kind existed - the depth limit's included
static void precedence()
{
  int n = 0, taken = 0;
  for (int slices = 0; slices <= 2; ++slices)
    for (int iso = 0; iso <= 2; ++iso)
      for (int projection = 0; projection <= 3; ++projection)
        for (int shading = 0; shading <= 2; ++shading)
          for (int pre = 0; pre <= 1; ++pre)
            for (int gradop = 0; gradop <= 1; ++gradop)
              for (int md = 0; md <= 1; ++md)
                for (int bits = 0; bits < 512; ++bits) {
                  const int k = (bits & 64) ? 3 : -1;
                  LaunchFacts f = small(bits & 64 ? 2 : 4);
                  f.shading = shading; f.projection = projection; f.slices = slices; f.isosurfaces = iso; f.preintegrated = pre != 0; f.gradient_opacity = gradop != 0; f.max_depth = md != 0;
                  f.pool = bits & 1; f.skipping = bits & 2; f.sparse = bits & 4; f.clip_on = bits & 8; f.lds_staging = bits & 16; f.slice_context = bits & 32; f.isosurface_context = bits & 32;
                  f.ranges = bits & 128; f.orthographic = bits & 256;
                  const LaunchPlan off = plan_launch(f, ov(k));
                  CHECK(!off.depth_output.on && off.depth_output.lds_bytes == 0 && !off.depth_output.limited && frame_kind(off) != FrameKind::DepthOutputMarch,
                        "slices %d isovalues %d projection %d shading %d pre %d gradop %d md %d bits %d: the kind without the fact", slices, iso, projection, shading, pre, gradop, md, bits);
                  f.depth_output = true; f.depth_threshold = 0.25f;
                  const LaunchPlan on = plan_launch(f, ov(k));
                  const bool march = slices == 0 && iso == 0 && projection == 0;
                  const bool preintegrated = march && shading == 0 && pre != 0; // pre-integration's own rule
                  const bool gradient_opacity = gradient_opacity_active(gradop, march, shading, preintegrated); // gradient opacity's own rule
                  const bool want = depth_output_active(true, march, shading, preintegrated, gradient_opacity);
                  CHECK(want == (march && shading <= 1 && !preintegrated && !gradient_opacity), "the host header's rule, spelled out");
                  if (want) {
                    CHECK(on.depth_output.on && frame_kind(on) == FrameKind::DepthOutputMarch && !on.error && on.depth_output.shade == (shading == 1) && on.depth_output.limited == (md != 0) && !on.max_depth.on,
                          "shading %d md %d bits %d: taken, in front of the depth limit", shading, md, bits);
                    CHECK((frame_kind(off) == FrameKind::DepthLimitedMarch) == (md != 0), "shading %d md %d bits %d: the depth limit alone plans its own kind", shading, md, bits);
                    ++taken;
                  }
                  else // kept and not drawn: the plan of the facts without it, member for member
                    CHECK(!on.depth_output.on && same_plan(on, off) && same_kinds(on, off) && frame_kind(on) == frame_kind(off),
                          "slices %d isovalues %d projection %d shading %d pre %d gradop %d md %d bits %d: kept, not drawn", slices, iso, projection, shading, pre, gradop, md, bits);
                  ++n;
                }
  CHECK(n == 3 * 3 * 4 * 3 * 2 * 2 * 2 * 512 && taken == 3 * 2 * 512, "%d plans, %d taken", n, taken);
  LaunchFacts f = small();
  f.max_depth = true;
  LaunchPlan p = plan_launch(f);
  CHECK(!p.error && frame_kind(p) == FrameKind::DepthLimitedMarch && p.max_depth.on && !p.depth_output.on, "the depth limit alone still plans DepthLimitedMarch");
  f.depth_output = true;
  p = plan_launch(f);
  CHECK(!p.error && frame_kind(p) == FrameKind::DepthOutputMarch && p.depth_output.limited && !p.max_depth.on, "both together plan the new kind with `limited`");
  f.shading = 2;
  p = plan_launch(f);
  CHECK(!p.error && !p.depth_output.on && !p.max_depth.on && frame_kind(p) == FrameKind::March && p.shading == 2, "FULL shading: both kept, not drawn");
  f = small(); f.depth_output = true; f.slices = 1;
  p = plan_launch(f);
  CHECK(!p.error && p.slices.on && !p.depth_output.on && p.march_lds_bytes == 384, "one plane under depth output: lds %zu", p.march_lds_bytes);
  // the new kind stands behind the twelve the other drivers loop over
  CHECK((int)FrameKind::DepthOutputMarch == (int)FrameKind::DepthLimitedMarch + 1 && (int)FrameKind::DepthLimitedMarch == (int)FrameKind::GradientOpacityMarch + 1
          && (int)FrameKind::GradientOpacityMarch == (int)FrameKind::PreintegratedMarch + 1 && (int)FrameKind::March == 0 && (int)FrameKind::DepthOutputMarch == 12,
        "appended last");
}

// the known-answer row: behind the depth limit's, its refusals in order, its record
static void query_row()
{
  CHECK(kRayQueryCount == 7 && kQueryPreintegrated == 7 && kQueryGradientOpacity == 8 && kQueryMaxDepth == 9 && kRayQueryAll == 10 && kQueryDepthOutput == 10 && kRayQueryTotal == 11,
        "the rows in front keep their ids");
  const RayQuery& d = ray_query_row(kQueryDepthOutput);
  CHECK(&d == &kDepthOutputQueries[0] && &ray_query_row(kQueryMaxDepth) == &kMaxDepthQueries[0] && &ray_query_row(kQueryGradientOpacity) == &kGradientOpacityQueries[0]
          && &ray_query_row(kQueryPreintegrated) == &kPreintegrationQueries[0] && &ray_query_row(kQuerySliceContext) == &kRayQueries[kQuerySliceContext],
        "the lookup");
  CHECK(!strcmp(d.name, "ovr_hip_depth_output_floats") && d.kind == FrameKind::DepthOutputMarch && d.needs == QueryNeeds::Nothing && d.takes_depth && d.depth_optional && d.takes_threshold && d.takes_shade
          && d.needs_tf && !d.needs_gradient_opacity && !d.needs_preintegration && !d.needs_context && !d.needs_ao && !d.takes_range_skipping && !d.takes_max_events && !d.takes_rotation && !d.takes_mode
          && !d.zeroed,
        "the row");
  for (int k = 0; k < kRayQueryAll; ++k) CHECK(!ray_query_row(k).takes_threshold && !ray_query_row(k).depth_optional, "row %d: the trailing members' defaults", k);
  CHECK(ray_query_record_floats(d, 0) == 12 && ray_query_record_floats(d, 16) == 12, "12 floats per ray");
  CHECK(query_runs(d, FrameKind::DepthOutputMarch) && !query_runs(d, FrameKind::March) && !query_runs(d, FrameKind::DepthLimitedMarch), "its own kind alone");
  QueryFacts f;
  QueryStatus s = ray_query_preconditions(d, f, false);
  CHECK(s.code == -3 && s.message == "[hip] ovr_hip_depth_output_floats: no volume was set", "%d %s", s.code, s.message.c_str());
  f.volume = true;
  s = ray_query_preconditions(d, f, false);
  CHECK(s.code == -3 && s.message == "[hip] ovr_hip_depth_output_floats: no transfer function was committed", "%d %s", s.code, s.message.c_str());
  f.transfer_function = true;
  CHECK(ray_query_preconditions(d, f, false).code == 0, "granted");
  f.slices = 2; f.isovalues = 3; f.preintegration = true; f.gradient_opacity = true;
  CHECK(ray_query_preconditions(d, f, false).code == 0, "granted under committed slices, isovalues, pre-integration and gradient opacity");
  // arguments: the depths are optional, the threshold is not
  RayQueryCall c;
  const float x = 0.f;
  float y = 0.f;
  c.org = &x; c.dir = &x; c.out = &y; c.n = 0;
  s = ray_query_arguments(d, true, c);
  CHECK(s.code == -1 && s.message == "[hip] ovr_hip_depth_output_floats: bad arguments", "threshold 0: %d %s", s.code, s.message.c_str());
  c.threshold = 0.5f;
  CHECK(ray_query_arguments(d, true, c).code == 0 && ray_query_arguments(d, false, c).code == -1, "no depths: no limit on any ray");
  c.depth = &x;
  CHECK(ray_query_arguments(d, true, c).code == 0, "depths");
  c.threshold = std::numeric_limits<float>::quiet_NaN();
  CHECK(ray_query_arguments(d, true, c).code == -1, "NaN");
  c.threshold = 1.f;
  CHECK(ray_query_arguments(d, true, c).code == -1, "above 0.9999f");
  c.threshold = 0.9999f; c.mode = 1;
  CHECK(ray_query_arguments(d, true, c).code == 0, "0.9999f, shade 1");
  c.mode = 2;
  CHECK(ray_query_arguments(d, true, c).code == -1, "shade 2");
  c.mode = 0; c.n = -1;
  CHECK(ray_query_arguments(d, true, c).code == -1, "n < 0");
  c.n = 0; c.out = nullptr;
  CHECK(ray_query_arguments(d, true, c).code == -1, "no out");
  // the depth limit's entry still needs its depths, and reads no threshold
  RayQueryCall g;
  g.org = &x; g.dir = &x; g.out = &y;
  CHECK(ray_query_arguments(ray_query_row(kQueryMaxDepth), true, g).code == -1, "ovr_hip_max_depth_floats without depths");
  g.depth = &x;
  CHECK(ray_query_arguments(ray_query_row(kQueryMaxDepth), true, g).code == 0, "... and with");
}

// ovr_hip_set_depth_output is recorded under kShading, like the other frame kinds: the accumulation starts over, nothing else is voided
static void commit_row()
{
  using namespace commit;
  for (int differs = 0; differs <= 1; ++differs) {
    Changes c;
    c.note(kShading, true, differs != 0); // every call resets, whether or not a value differs
    CommitFacts facts;
    facts.framebuffer = facts.volume = true;
    const Effects e = plan_commit(c, facts);
    CHECK(e.has(kReset) && e.what == kChanged, "the accumulation starts over and nothing else follows: %#x", e.what);
    CHECK(!e.has(kResort) && !e.has(kRelist) && !e.has(kMajorantVoid) && !e.has(kRangesVoid) && !e.has(kLatticeStale) && !e.has(kSkipRestart), "nothing is voided: %#x", e.what);
  }
  Changes none;
  CommitFacts facts;
  facts.framebuffer = facts.volume = true;
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
  if (argc == 10 && !strcmp(argv[1], "rule")) {
    LaunchFacts f = small();
    f.depth_output = std::atoi(argv[2]) != 0; f.depth_threshold = 0.5f;
    f.slices = std::atoi(argv[3]); f.isosurfaces = std::atoi(argv[4]); f.projection = std::atoi(argv[5]); f.shading = std::atoi(argv[6]);
    f.preintegrated = std::atoi(argv[7]) != 0; f.gradient_opacity = std::atoi(argv[8]) != 0; f.max_depth = std::atoi(argv[9]) != 0;
    const LaunchPlan p = plan_launch(f);
    printf("%d %d\n", p.error ? -1 : (int)frame_kind(p), p.depth_output.limited ? 1 : 0);
    return 0;
  }
  for (const Scenario& s : kScenarios)
    if (argc == 2 && !strcmp(argv[1], s.name)) {
      s.run();
      if (g_failed) printf("%d checks failed\n", g_failed);
      return g_failed ? 1 : 0;
    }
  printf("usage: driver --list | <scenario> | rule <on> <slices> <isovalues> <projection> <shading> <pre> <gradop> <max_depth>\n");
  return 2;
}
