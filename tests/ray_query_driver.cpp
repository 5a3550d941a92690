// Driver of tests/test_ray_query_table.py: the table of the known-answer ray queries (csrc/host/ray_query.hpp) and frame_kind (csrc/host/launch_plan.hpp) on the
// CPU.  `driver <scenario>` exits 0 when every row gave what it expects.  The messages, codes and sizes are literals - what each of the seven entries of
// ovr_hip_api.cpp returned when it was written out by hand -, none is put together from the table under test.
#include "launch_plan.hpp"
#include "ray_query.hpp"

#include <cstdio>
#include <cstring>

using namespace ovrhip;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } \
  } while (0)

// ---- part one: the table
// an entry's refusals, in the order it reports them; nullptr: the entry does not ask
struct Expect { RayQueryId id; const char* arguments; const char* volume; const char* committed; const char* context; const char* ao; const char* tf; const char* ranges; };
static const Expect kExpect[] = {
  { kQueryProject, "[hip] ovr_hip_project_floats: bad arguments", "[hip] ovr_hip_project_floats: no volume was set", nullptr, nullptr, nullptr, nullptr,
    "[hip] ovr_hip_project_floats: the resident volume has no macrocell ranges" },
  { kQuerySlice, "[hip] ovr_hip_slice_floats: bad arguments", "[hip] ovr_hip_slice_floats: no volume was set", "[hip] ovr_hip_slice_floats: no slice is committed (ovr_hip_set_slices)",
    nullptr, nullptr, nullptr, "[hip] ovr_hip_slice_floats: the resident volume has no macrocell ranges" },
  { kQuerySliceContext, "[hip] ovr_hip_slice_context_floats: bad arguments", "[hip] ovr_hip_slice_context_floats: no volume was set",
    "[hip] ovr_hip_slice_context_floats: no slice is committed (ovr_hip_set_slices)", "[hip] ovr_hip_slice_context_floats: no slice context is committed (ovr_hip_set_slice_context)", nullptr,
    "[hip] ovr_hip_slice_context_floats: no transfer function was committed", nullptr },
  { kQueryIsosurface, "[hip] ovr_hip_isosurface_floats: bad arguments", "[hip] ovr_hip_isosurface_floats: no volume was set",
    "[hip] ovr_hip_isosurface_floats: no isovalue is committed (ovr_hip_set_isosurfaces)", nullptr, nullptr, nullptr, "[hip] ovr_hip_isosurface_floats: the resident volume has no macrocell ranges" },
  { kQueryIsosurfaceLayers, "[hip] ovr_hip_isosurface_layers_floats: bad arguments", "[hip] ovr_hip_isosurface_layers_floats: no volume was set",
    "[hip] ovr_hip_isosurface_layers_floats: no isovalue is committed (ovr_hip_set_isosurface_layers)", nullptr, nullptr, nullptr,
    "[hip] ovr_hip_isosurface_layers_floats: the resident volume has no macrocell ranges" },
  { kQueryIsosurfaceContext, "[hip] ovr_hip_isosurface_context_floats: bad arguments", "[hip] ovr_hip_isosurface_context_floats: no volume was set",
    "[hip] ovr_hip_isosurface_context_floats: no isovalue is committed (ovr_hip_set_isosurfaces)",
    "[hip] ovr_hip_isosurface_context_floats: no isosurface context is committed (ovr_hip_set_isosurface_context)", nullptr,
    "[hip] ovr_hip_isosurface_context_floats: no transfer function was committed", nullptr },
  { kQueryIsosurfaceAo, "[hip] ovr_hip_isosurface_ao_floats: bad arguments", "[hip] ovr_hip_isosurface_ao_floats: no volume was set",
    "[hip] ovr_hip_isosurface_ao_floats: no isovalue is committed (ovr_hip_set_isosurface_layers)", nullptr,
    "[hip] ovr_hip_isosurface_ao_floats: no ambient-occlusion sample is committed (ovr_hip_set_ambient_occlusion)", nullptr,
    "[hip] ovr_hip_isosurface_ao_floats: the resident volume has no macrocell ranges" },
};
constexpr int kEinval = -1, kEstate = -3; // include/ovr_hip.h

enum Fact { kVolume, kCommitted, kContext, kAo, kTf, kRanges, kFacts };
static const char* expected(const Expect& e, int fact)
{
  const char* const m[kFacts] = { e.volume, e.committed, e.context, e.ao, e.tf, e.ranges };
  return m[fact];
}
// the committed facts with the ones of `met` met (a bit per Fact): slices and isovalues, and both contexts, go together - an entry reads its own
static QueryFacts facts(unsigned met)
{
  QueryFacts f;
  f.volume = met & (1u << kVolume);
  f.slices = f.isovalues = (met & (1u << kCommitted)) ? 2 : 0;
  f.slice_context = f.isosurface_context = met & (1u << kContext);
  f.ao_samples = (met & (1u << kAo)) ? 4 : 0;
  f.transfer_function = met & (1u << kTf);
  f.ranges = met & (1u << kRanges);
  return f;
}
static bool is(const QueryStatus& s, int code, const char* message) { return message ? s.code == code && s.message == message : s.code == 0 && s.message.empty(); }

static void preconditions()
{
  CHECK(sizeof(kExpect) / sizeof(kExpect[0]) == kRayQueryCount, "seven entries");
  const unsigned all = (1u << kFacts) - 1;
  for (const Expect& e : kExpect) {
    const RayQuery& d = kRayQueries[e.id];
    CHECK(is(ray_query_preconditions(d, facts(all), true), 0, nullptr), "%s: everything met", d.name);
    // one precondition unmet, everything else met: its message, or none where the entry does not ask
    for (int k = 0; k < kFacts; ++k) {
      const QueryStatus s = ray_query_preconditions(d, facts(all & ~(1u << k)), true);
      CHECK(is(s, kEstate, expected(e, k)), "%s without fact %d: %d '%s'", d.name, k, s.code, s.message.c_str());
    }
    // the order: nothing met, then one more at a time - always the first unmet one the entry asks about
    unsigned met = 0;
    for (int k = 0; k <= kFacts; ++k) {
      const char* first = nullptr;
      for (int j = kFacts - 1; j >= 0; --j)
        if (!(met & (1u << j)) && expected(e, j)) first = expected(e, j);
      const QueryStatus s = ray_query_preconditions(d, facts(met), true);
      CHECK(is(s, kEstate, first), "%s with the first %d facts met: %d '%s'", d.name, k, s.code, s.message.c_str());
      met |= 1u << k;
    }
    // without range skipping nobody asks for the ranges
    CHECK(is(ray_query_preconditions(d, facts(all & ~(1u << kRanges)), false), 0, nullptr), "%s: no skipping, no ranges", d.name);
  }
}

static void arguments()
{
  const float x = 0.f;
  float y = 0.f;
  for (const Expect& e : kExpect) {
    const RayQuery& d = kRayQueries[e.id];
    RayQueryCall ok;
    ok.org = ok.dir = &x; ok.out = &y; ok.n = 5; ok.mode = 1; ok.max_events = 8; ok.rotation = 3; ok.range_skipping = 1;
    CHECK(is(ray_query_arguments(d, true, ok), 0, nullptr), "%s: a good call", d.name);
    RayQueryCall c = ok;
    c.n = 0;
    CHECK(is(ray_query_arguments(d, true, c), 0, nullptr), "%s: no rays", d.name);
    CHECK(is(ray_query_arguments(d, false, ok), kEinval, e.arguments), "%s: no renderer", d.name);
    c = ok; c.org = nullptr;
    CHECK(is(ray_query_arguments(d, true, c), kEinval, e.arguments), "%s: no origins", d.name);
    c = ok; c.dir = nullptr;
    CHECK(is(ray_query_arguments(d, true, c), kEinval, e.arguments), "%s: no directions", d.name);
    c = ok; c.out = nullptr;
    CHECK(is(ray_query_arguments(d, true, c), kEinval, e.arguments), "%s: no output", d.name);
    c = ok; c.n = -1;
    CHECK(is(ray_query_arguments(d, true, c), kEinval, e.arguments), "%s: n < 0", d.name);
    // the arguments an entry takes are held to their ranges, the others are not read: mode 1 ... 3 (the projection alone), max_events 1 ... 16 (the three
    // entries with events), rotation 0 ... 15 (the AO entry alone)
    const bool mode = e.id == kQueryProject, events = e.id == kQueryIsosurfaceLayers || e.id == kQueryIsosurfaceContext || e.id == kQueryIsosurfaceAo, rotation = e.id == kQueryIsosurfaceAo;
    for (int v : { 0, 4 }) { c = ok; c.mode = v; CHECK(is(ray_query_arguments(d, true, c), kEinval, mode ? e.arguments : nullptr), "%s: mode %d", d.name, v); }
    for (int v : { 1, 3 }) { c = ok; c.mode = v; CHECK(is(ray_query_arguments(d, true, c), 0, nullptr), "%s: mode %d", d.name, v); }
    for (int v : { 0, 17, -1 }) { c = ok; c.max_events = v; CHECK(is(ray_query_arguments(d, true, c), kEinval, events ? e.arguments : nullptr), "%s: max_events %d", d.name, v); }
    for (int v : { 1, 16 }) { c = ok; c.max_events = v; CHECK(is(ray_query_arguments(d, true, c), 0, nullptr), "%s: max_events %d", d.name, v); }
    for (int v : { -1, 16 }) { c = ok; c.rotation = v; CHECK(is(ray_query_arguments(d, true, c), kEinval, rotation ? e.arguments : nullptr), "%s: rotation %d", d.name, v); }
    for (int v : { 0, 15 }) { c = ok; c.rotation = v; CHECK(is(ray_query_arguments(d, true, c), 0, nullptr), "%s: rotation %d", d.name, v); }
  }
}

// floats per ray: 4, 4, 8, 8, 4 + 8 E, 8 + 8 E, 8 + 8 E; which outputs are zeroed first; which frame kind's twin runs
static void records()
{
  struct Row { RayQueryId id; size_t at1, at8, at16; bool zeroed; FrameKind kind; };
  const Row t[] = {
    { kQueryProject, 4, 4, 4, false, FrameKind::Projection },
    { kQuerySlice, 4, 4, 4, false, FrameKind::SliceWalk },
    { kQuerySliceContext, 8, 8, 8, false, FrameKind::SliceContext },
    { kQueryIsosurface, 8, 8, 8, false, FrameKind::Isosurface },
    { kQueryIsosurfaceLayers, 12, 68, 132, true, FrameKind::IsosurfaceLayers },
    { kQueryIsosurfaceContext, 16, 72, 136, true, FrameKind::IsosurfaceContext },
    { kQueryIsosurfaceAo, 16, 72, 136, true, FrameKind::IsosurfaceAo },
  };
  CHECK(sizeof(t) / sizeof(t[0]) == kRayQueryCount, "seven entries");
  for (const Row& r : t) {
    const RayQuery& d = kRayQueries[r.id];
    CHECK(ray_query_record_floats(d, 1) == r.at1 && ray_query_record_floats(d, 8) == r.at8 && ray_query_record_floats(d, 16) == r.at16, "%s: %zu / %zu / %zu floats", d.name,
          ray_query_record_floats(d, 1), ray_query_record_floats(d, 8), ray_query_record_floats(d, 16));
    CHECK(d.zeroed == r.zeroed && d.kind == r.kind, "%s: zeroed %d kind %d", d.name, (int)d.zeroed, (int)d.kind);
    // a query runs the plan of its own kind and no other - but the slices' entry, whose committed set decides between the plane and the walk kernel
    for (int k = (int)FrameKind::March; k <= (int)FrameKind::SliceContext; ++k)
      CHECK(query_runs(d, (FrameKind)k) == ((FrameKind)k == r.kind || (r.id == kQuerySlice && (FrameKind)k == FrameKind::SlicePlane)), "%s under a plan of kind %d", d.name, k);
  }
}

// ---- part two: frame_kind
static LaunchFacts small()
{
  LaunchFacts f;
  f.elem_bytes = 4; f.f32_general = true;
  f.nx = 40; f.ny = 33; f.nz = 18;
  f.stored_bytes = 1u << 20;
  f.n_color = f.n_alpha = 256;
  f.n_blocks_owned = f.n_schedule = 20;
  return f;
}

// the precedence cases by hand: projection mode, isovalues, slices, a slab among them, slice context, isosurface context, AO samples, translucent, shading -> kind
static void precedence_table()
{
  struct Row { int projection, iso, slices; bool walks, slice_ctx, iso_ctx, ao, translucent; int shading; FrameKind kind; };
  const Row t[] = {
    { 0, 0, 0, false, false, false, false, false, 2, FrameKind::March },
    { 0, 0, 0, true, true, true, true, true, 2, FrameKind::March },          // everything kept, nothing committed to draw
    { 3, 0, 0, false, true, true, true, true, 1, FrameKind::Projection },
    { 1, 2, 0, false, false, false, false, false, 2, FrameKind::Isosurface }, // isovalues over a projection mode
    { 0, 1, 0, false, true, false, false, false, 0, FrameKind::Isosurface },  // the slice context is not an isosurface frame's
    { 2, 2, 0, false, false, false, false, true, 0, FrameKind::IsosurfaceLayers },
    { 0, 2, 0, false, false, false, true, false, 0, FrameKind::Isosurface },  // no ambient term without shading: the samples are kept
    { 0, 2, 0, false, false, false, true, true, 0, FrameKind::IsosurfaceLayers },
    { 0, 2, 0, false, false, false, true, false, 1, FrameKind::IsosurfaceAo }, // opaque: the AO twin of the translucent kernel
    { 0, 4, 0, false, false, false, true, true, 2, FrameKind::IsosurfaceAo },
    { 0, 1, 0, false, false, true, false, false, 0, FrameKind::IsosurfaceContext },
    { 3, 3, 0, true, true, true, true, true, 2, FrameKind::IsosurfaceContext }, // the context over AO and the layers
    { 0, 0, 1, false, false, false, false, false, 0, FrameKind::SlicePlane },
    { 2, 4, 1, false, false, true, true, true, 2, FrameKind::SlicePlane },     // slices over isovalues, their context and their AO
    { 0, 0, 3, true, false, false, false, false, 1, FrameKind::SliceWalk },
    { 1, 2, 4, true, false, true, true, false, 2, FrameKind::SliceWalk },
    { 0, 0, 1, false, true, false, false, false, 0, FrameKind::SliceContext },
    { 0, 0, 2, true, true, false, false, false, 2, FrameKind::SliceContext },  // one context kernel for planes and slabs
    { 3, 4, 4, true, true, true, true, true, 2, FrameKind::SliceContext },
  };
  for (const Row& r : t) {
    LaunchFacts f = small();
    f.projection = r.projection; f.isosurfaces = r.iso; f.slices = r.slices; f.slice_walks = r.walks; f.slice_extremum = r.walks; f.slice_context = r.slice_ctx;
    f.isosurface_context = r.iso_ctx; f.ambient_occlusion = r.ao; f.translucent = r.translucent; f.shading = r.shading;
    const LaunchPlan p = plan_launch(f);
    CHECK(!p.error && frame_kind(p) == r.kind && plan_variants_exist(p, true), "projection %d isovalues %d slices %d walks %d contexts %d %d ao %d translucent %d shading %d: kind %d",
          r.projection, r.iso, r.slices, (int)r.walks, (int)r.slice_ctx, (int)r.iso_ctx, (int)r.ao, (int)r.translucent, r.shading, (int)frame_kind(p));
  }
  // the committed state's own statement
  CHECK(committed_frame(0, 0, 0) == CommittedFrame::March && committed_frame(0, 0, 2) == CommittedFrame::Projection && committed_frame(0, 3, 2) == CommittedFrame::Isovalues
          && committed_frame(0, 1, 0) == CommittedFrame::Isovalues && committed_frame(2, 3, 1) == CommittedFrame::Slices && committed_frame(1, 0, 0) == CommittedFrame::Slices,
        "slices over isovalues over projection over march");
  // an error plan reads as the march and names no variant
  LaunchFacts f = small();
  f.slices = 5;
  CHECK(plan_launch(f).error && frame_kind(plan_launch(f)) == FrameKind::March && !plan_variants_exist(plan_launch(f), true), "five slices");
}

// the grid the plan drivers sweep: every plan's kind is the kind of its facts - restated here on the facts, in the plan's own words nowhere - and its variant exists
static FrameKind kind_of_facts(const LaunchFacts& f)
{
  if (f.slices > 0) return f.slice_context ? FrameKind::SliceContext : f.slice_walks ? FrameKind::SliceWalk : FrameKind::SlicePlane;
  if (f.isosurfaces > 0) {
    if (f.isosurface_context) return FrameKind::IsosurfaceContext;
    if (f.ambient_occlusion && f.shading != 0) return FrameKind::IsosurfaceAo;
    return f.translucent ? FrameKind::IsosurfaceLayers : FrameKind::Isosurface;
  }
  return f.projection != 0 ? FrameKind::Projection : FrameKind::March;
}
static void grid()
{
  int n = 0, seen[9] = { 0 };
  for (int projection = 0; projection <= 3; ++projection)
    for (int iso = 0; iso <= 4; ++iso)
      for (int slices = 0; slices <= 4; ++slices)
        for (int shading = 0; shading <= 2; ++shading)
          for (int bits = 0; bits < 256; ++bits) {
            LaunchFacts f = small();
            f.projection = projection; f.isosurfaces = iso; f.slices = slices; f.shading = shading;
            f.slice_walks = f.slice_extremum = bits & 1; f.slice_context = bits & 2; f.isosurface_context = bits & 4; f.ambient_occlusion = bits & 8; f.translucent = bits & 16;
            f.clip_on = bits & 32; f.orthographic = bits & 64; f.ranges = f.skipping = bits & 128;
            const LaunchPlan p = plan_launch(f);
            const FrameKind k = frame_kind(p);
            CHECK(!p.error && k == kind_of_facts(f), "projection %d isovalues %d slices %d shading %d bits %d: kind %d", projection, iso, slices, shading, bits, (int)k);
            CHECK(plan_variants_exist(p, true), "projection %d isovalues %d slices %d shading %d bits %d: the plan names a variant that does not exist", projection, iso, slices, shading, bits);
            ++seen[(int)k];
            ++n;
          }
  CHECK(n == 4 * 5 * 5 * 3 * 256, "%d plans", n);
  for (int k = 0; k < 9; ++k) CHECK(seen[k] > 0, "no plan of kind %d", k);
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "preconditions", preconditions }, { "arguments", arguments }, { "records", records }, { "precedence_table", precedence_table }, { "grid", grid } };

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
