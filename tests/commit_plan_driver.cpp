// Driver of tests/test_commit_plan.py: runs csrc/host/commit_plan.hpp - what a changed parameter invalidates - on the CPU.  `driver <scenario>` exits 0 when
// every row of the scenario gave what it expects.  The expectations are literals, written by reading the commit as it was before the table existed (one
// function of flag assignments) and the flag blocks of the volume upload, ovr_hip_update_volume, the noise tile and the supplied shadow values; none is
// computed from the header's table.
#include "commit_plan.hpp"

#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace ovrhip::commit;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } \
  } while (0)

// what the commit did after ANY change it counted as one: reset, the clear generation, the pool unproven, the estimate void
constexpr unsigned C = kReset | kBumpClearGen | kPoolUnproven | kEstimateVoid;

// per source: set with a new value, set with the same value again.  (With a framebuffer and a volume, no reset pending, the camera derived.)
struct Expect { Source source; const char* name; unsigned fresh; Tuner fresh_tuner; unsigned same; Tuner same_tuner; };
static const Expect kExpect[] = {
  { kFramebuffer, "framebuffer", C | kResort | kCameraParams, kTunerChanged, C | kResort | kCameraParams, kTunerChanged },
  { kCamera, "camera", C | kResort | kCameraParams, kTunerCameraMoved, C | kResort | kCameraParams, kTunerCameraMoved },
  { kTransferFunction, "transfer function", C | kMajorantVoid | kLatticeStale, kTunerChanged, C | kMajorantVoid | kLatticeStale, kTunerChanged },
  { kGridConvention, "grid convention", C | kResort | kVolumeParams | kLatticeStale, kTunerChanged, C | kResort | kVolumeParams | kLatticeStale, kTunerChanged },
  { kFocus, "focus", C, kTunerChanged, C, kTunerChanged },
  { kSpp, "spp", C | kResort, kTunerChanged, C | kResort, kTunerChanged },
  { kSparse, "sparse sampling", C, kTunerChanged, C, kTunerChanged },
  { kAccumulation, "accumulation", C, kTunerChanged, C, kTunerChanged },
  { kSamplingRate, "sampling rate", C | kLatticeStale, kTunerChanged, C, kTunerChanged },
  { kShading, "shading", C, kTunerChanged, C, kTunerChanged },
  { kJitter, "jitter", C | kResort, kTunerChanged, C | kResort, kTunerChanged },
  { kConvergence, "convergence", C | kFreeConvergence, kTunerChanged, C, kTunerChanged },
  { kReconstruction, "reconstruction", C | kFreeReconstruction, kTunerChanged, C, kTunerChanged },
  { kLightVector, "light vector", C | kLighting, kTunerChanged, kLighting, kTunerKeeps },
  { kLightDirection, "light direction", kLatticeStale, kTunerKeeps, 0, kTunerKeeps },
  { kLightIntensity, "light intensity", C, kTunerChanged, 0, kTunerKeeps },
  { kMaterial, "material", C | kLighting, kTunerChanged, kLighting, kTunerKeeps },
  { kClipBox, "clip box", C | kResort | kLatticeStale | kClipParams, kTunerChanged, kClipParams, kTunerKeeps },
  { kShadowMode, "shadow mode", C | kLatticeStale, kTunerVoid, 0, kTunerKeeps },
  { kShadowCell, "shadow cell", C | kLatticeStale, kTunerChanged, 0, kTunerKeeps },
  { kShadowLeavesSupplied, "shadow mode leaves SUPPLIED", kFreeSuppliedLattice, kTunerKeeps, 0, kTunerKeeps },
  { kShadowEntersMarched, "shadow mode enters MARCHED", kFreeBuiltLattice, kTunerKeeps, 0, kTunerKeeps },
  { kLdsStaging, "LDS staging", 0, kTunerKeeps, 0, kTunerKeeps },
  { kLayoutChoice, "layout choice", 0, kTunerVoid, 0, kTunerKeeps },
  { kPipeline, "pipeline", 0, kTunerVoid, 0, kTunerKeeps },
  { kSkipping, "skipping", kSkipRestart, kTunerKeeps, kSkipRestart, kTunerKeeps },
  { kShard, "image shard", C | kRelist, kTunerChanged, C | kRelist, kTunerChanged },
  // the calls that are no commit: no clear generation; the upload leaves the estimate; state = 0, not a restart
  { kVolumeUpload, "volume upload", kReset | kResort | kPoolUnproven | kRangesVoid | kMajorantVoid | kLatticeStale | kVolumeParams, kTunerStateZero,
    kReset | kResort | kPoolUnproven | kRangesVoid | kMajorantVoid | kLatticeStale | kVolumeParams, kTunerStateZero },
  { kVolumeUpdate, "volume update", kReset | kEstimateVoid | kPoolUnproven | kMajorantVoid | kLatticeStale, kTunerStateZero,
    kReset | kEstimateVoid | kPoolUnproven | kMajorantVoid | kLatticeStale, kTunerStateZero },
  { kNoiseTile, "noise tile", kReset, kTunerKeeps, kReset, kTunerKeeps },
  { kShadowValues, "supplied shadow values", kReset, kTunerKeeps, 0, kTunerKeeps }, // (differs: the committed mode reads them)
};
constexpr int kExpected = (int)(sizeof(kExpect) / sizeof(kExpect[0]));

static CommitFacts usual()
{
  CommitFacts f;
  f.framebuffer = f.volume = true;
  return f;
}
static const Expect& expect(Source s)
{
  for (const Expect& e : kExpect)
    if (e.source == s) return e;
  g_failed++;
  printf("FAILED: source %d has no expectation\n", (int)s);
  return kExpect[0];
}
static bool every_source_once()
{
  int seen[kSourceCount] = {};
  for (const Expect& e : kExpect) seen[e.source]++;
  for (int s = 0; s < kSourceCount; ++s)
    if (seen[s] != 1) return false;
  return kExpected == kSourceCount;
}

static void single(bool fresh)
{
  CHECK(every_source_once(), "the table lists every source once (%d rows, %d sources)", kExpected, (int)kSourceCount);
  for (const Expect& x : kExpect) {
    Changes c;
    c.note(x.source, true, fresh);
    const Effects e = plan_commit(c, usual());
    const unsigned want = fresh ? x.fresh : x.same;
    const Tuner tuner = fresh ? x.fresh_tuner : x.same_tuner;
    CHECK(e.what == want && e.tuner == tuner, "%s, %s value: effects %#x tuner %d, expected %#x tuner %d", x.name, fresh ? "a new" : "the same", e.what, (int)e.tuner, want, (int)tuner);
    // a value that was not set does nothing, whatever `differs` says
    Changes n;
    n.of[x.source].differs = true;
    n.note(x.source, false, true);
    CHECK(plan_commit(n, usual()).what == 0 && plan_commit(n, usual()).tuner == kTunerKeeps, "%s, not set: effects", x.name);
  }
}
static void single_new() { single(true); }
static void single_same() { single(false); }

static void nothing_set()
{
  const Effects e = plan_commit(Changes(), usual());
  CHECK(e.what == 0 && e.tuner == kTunerKeeps && !e.has(kBumpClearGen) && !e.has(kReset), "nothing set: effects %#x tuner %d", e.what, (int)e.tuner);
  CHECK(plan_commit(Changes(), CommitFacts()).what == 0, "nothing set, no framebuffer, no volume");
}

static void pending_reset()
{
  CommitFacts f = usual();
  f.reset_pending = true;
  const Effects e = plan_commit(Changes(), f);
  // the commit voided the estimate whenever it left the flag set - and touched nothing else: no clear generation, the pool and the tuner as they were
  CHECK(e.what == (kReset | kEstimateVoid) && e.tuner == kTunerKeeps, "a pending reset alone: effects %#x tuner %d", e.what, (int)e.tuner);
  Changes c;
  c.note(kPipeline, true, true);
  const Effects p = plan_commit(c, f);
  CHECK(p.what == (kReset | kEstimateVoid) && p.tuner == kTunerVoid, "a pending reset and a new pipeline: effects %#x tuner %d", p.what, (int)p.tuner);
  c = Changes();
  c.note(kCamera, true, true);
  const Effects m = plan_commit(c, f);
  CHECK(m.what == (C | kResort | kCameraParams) && m.tuner == kTunerCameraMoved, "a pending reset and a camera: to the tuner still only the camera (%#x, %d)", m.what, (int)m.tuner);
}

static void camera_class()
{
  Changes cam;
  cam.note(kCamera, true, true);
  CHECK(plan_commit(cam, usual()).tuner == kTunerCameraMoved, "camera alone");
  // ... plus any source that resets: the configuration changed
  int resetting = 0;
  for (const Expect& x : kExpect) {
    if (x.source == kCamera || x.source >= kVolumeUpload || !(x.fresh & kReset)) continue;
    ++resetting;
    Changes c = cam;
    c.note(x.source, true, true);
    const Effects e = plan_commit(c, usual());
    const Tuner want = x.source == kShadowMode ? kTunerVoid : kTunerChanged;
    CHECK(e.tuner == want && e.has(kReset) && e.has(kBumpClearGen) && e.has(kCameraParams), "camera + %s: tuner %d, expected %d", x.name, (int)e.tuner, (int)want);
  }
  CHECK(resetting == 19, "the resetting sources of a commit besides the camera: %d", resetting);
  // a resized framebuffer counts as "other", with or without a camera
  Changes fb;
  fb.note(kFramebuffer, true, true);
  CHECK(plan_commit(fb, usual()).tuner == kTunerChanged, "framebuffer alone");
  fb.note(kCamera, true, true);
  CHECK(plan_commit(fb, usual()).tuner == kTunerChanged, "framebuffer + camera");
  // camera + a source that does not reset: still only the camera
  for (Source s : { kLdsStaging, kSkipping }) {
    Changes c = cam;
    c.note(s, true, true);
    CHECK(plan_commit(c, usual()).tuner == kTunerCameraMoved, "camera + source %d", (int)s);
  }
  Changes same = cam;
  same.note(kLightVector, true, false); same.note(kLightDirection, true, false); same.note(kLightIntensity, true, false);
  same.note(kMaterial, true, false); same.note(kClipBox, true, false); same.note(kShadowMode, true, false); same.note(kShadowCell, true, false);
  CHECK(plan_commit(same, usual()).tuner == kTunerCameraMoved, "camera + light, material, clip box and shadow cache set to what they were");
  // a camera that was never derived behaves as a camera that was set
  CommitFacts dirty = usual();
  dirty.camera_dirty = true;
  const Effects d = plan_commit(Changes(), dirty), c = plan_commit(cam, usual());
  CHECK(d.what == c.what && d.tuner == c.tuner && d.what == (C | kResort | kCameraParams), "camera_dirty alone: effects %#x tuner %d", d.what, (int)d.tuner);
  // ... and without a framebuffer nothing is derived (the camera stays dirty), everything else as usual
  dirty.framebuffer = false;
  const Effects n = plan_commit(Changes(), dirty);
  CHECK(n.what == (C | kResort) && n.tuner == kTunerCameraMoved, "camera_dirty, no framebuffer: effects %#x", n.what);
  // the grid convention without a volume derives nothing either
  Changes g;
  g.note(kGridConvention, true, true);
  CommitFacts nv = usual();
  nv.volume = false;
  CHECK(plan_commit(g, nv).what == (C | kResort | kLatticeStale), "grid convention, no volume: effects %#x", plan_commit(g, nv).what);
}

static void void_rule()
{
  for (Source s : { kLayoutChoice, kPipeline, kShadowMode }) {
    Changes c;
    c.note(s, true, true);
    const Effects e = plan_commit(c, usual());
    CHECK(e.tuner == kTunerVoid, "source %d, a new value: tuner %d", (int)s, (int)e.tuner);
    if (s != kShadowMode) CHECK(e.what == 0, "source %d, a new value: no reset, no clear generation (effects %#x)", (int)s, e.what);
    Changes same;
    same.note(s, true, false);
    const Effects k = plan_commit(same, usual());
    CHECK(k.tuner == kTunerKeeps && k.what == 0, "source %d, the same value: effects %#x tuner %d", (int)s, k.what, (int)k.tuner);
    // void wins over everything else that fired
    c.note(kCamera, true, true);
    CHECK(plan_commit(c, usual()).tuner == kTunerVoid, "source %d + camera", (int)s);
    c.note(kTransferFunction, true, true);
    CHECK(plan_commit(c, usual()).tuner == kTunerVoid, "source %d + camera + transfer function", (int)s);
  }
}

// the tuner's fate of several sources, by the stated rule
static Tuner combined(const Tuner* t, int n)
{
  bool camera = false, other = false, zero = false, voids = false;
  for (int i = 0; i < n; ++i) {
    camera |= t[i] == kTunerCameraMoved; other |= t[i] == kTunerChanged; zero |= t[i] == kTunerStateZero; voids |= t[i] == kTunerVoid;
  }
  return voids ? kTunerVoid : other ? kTunerChanged : zero ? kTunerStateZero : camera ? kTunerCameraMoved : kTunerKeeps;
}

// over every pair of sources (each new or the same) and a fixed-seed sample of larger subsets: the plan is the OR of the single-source expectations
static void sweep()
{
  long plans = 0;
  auto check = [&](const int* state /* per source: 0 not set, 1 the same value, 2 a new one */) {
    Changes c;
    unsigned want = 0;
    Tuner votes[kSourceCount];
    int n = 0;
    for (int s = 0; s < kSourceCount; ++s) {
      if (!state[s]) continue;
      c.note((Source)s, true, state[s] == 2);
      const Expect& x = expect((Source)s);
      want |= state[s] == 2 ? x.fresh : x.same;
      votes[n++] = state[s] == 2 ? x.fresh_tuner : x.same_tuner;
    }
    const Effects e = plan_commit(c, usual());
    ++plans;
    const Tuner tuner = combined(votes, n);
    if (e.what != want || e.tuner != tuner) {
      g_failed++;
      printf("FAILED: states");
      for (int s = 0; s < kSourceCount; ++s) printf(" %d", state[s]);
      printf(": effects %#x tuner %d, expected %#x tuner %d\n", e.what, (int)e.tuner, want, (int)tuner);
    }
  };
  for (int a = 0; a < kSourceCount; ++a)
    for (int b = a + 1; b < kSourceCount; ++b)
      for (int sa = 1; sa <= 2; ++sa)
        for (int sb = 1; sb <= 2; ++sb) {
          int state[kSourceCount] = {};
          state[a] = sa; state[b] = sb;
          check(state);
        }
  unsigned long long x = 0x9e3779b97f4a7c15ull; // xorshift64, fixed seed
  for (int i = 0; i < 20000; ++i) {
    int state[kSourceCount] = {};
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    const int density = 1 + (int)(x % 4); // sparse to dense subsets
    for (int s = 0; s < kSourceCount; ++s) {
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      state[s] = (int)((x >> 20) % 4) < density ? 1 + (int)((x >> 40) & 1) : 0;
    }
    check(state);
  }
  printf("sweep: %ld plans\n", plans);
  CHECK(plans == (long)kSourceCount * (kSourceCount - 1) / 2 * 4 + 20000, "the sweep's size");
}

// the staleness table of DESIGN.md section 14 (it was a rule of its own, with 22 flags, before it became a column): each change alone, and together with
// every change that does not count
static void shadow_staleness()
{
  struct Row { const char* what; Source source; bool stale; };
  const Row rows[] = {
    { "volume", kVolumeUpload, true }, { "update_volume", kVolumeUpdate, true }, { "transfer function", kTransferFunction, true },
    { "sampling rate", kSamplingRate, true }, { "light direction", kLightDirection, true }, { "clip box", kClipBox, true },
    { "grid convention", kGridConvention, true }, { "cell", kShadowCell, true }, { "mode", kShadowMode, true },
    { "camera", kCamera, false }, { "framebuffer", kFramebuffer, false }, { "spp", kSpp, false },
    { "jitter", kJitter, false }, { "material", kMaterial, false }, { "light intensity", kLightIntensity, false },
    { "accumulation", kAccumulation, false }, { "sparse sampling", kSparse, false }, { "convergence", kConvergence, false },
    { "reconstruction", kReconstruction, false }, { "layout choice", kLayoutChoice, false }, { "pipeline", kPipeline, false },
    { "skipping", kSkipping, false },
  };
  // the sources that had no flag: none of them makes the lattice stale either
  const Source rest[] = { kFocus, kShading, kLightVector, kShadowLeavesSupplied, kShadowEntersMarched, kLdsStaging, kShard, kNoiseTile, kShadowValues };
  auto stale = [](const Changes& c) { return plan_commit(c, usual()).has(kLatticeStale); };
  CHECK(!stale(Changes()), "nothing changed: stale");
  Changes neutral;
  for (const Row& r : rows)
    if (!r.stale) neutral.happened(r.source);
  CHECK(!stale(neutral), "every change that does not count, together: stale");
  int n_stale = 0, seen[kSourceCount] = {};
  for (const Row& r : rows) {
    Changes c;
    c.happened(r.source);
    CHECK(stale(c) == r.stale, "%s alone: stale %d, expected %d", r.what, (int)stale(c), (int)r.stale);
    Changes d = neutral;
    d.happened(r.source);
    CHECK(stale(d) == r.stale, "%s with the neutral changes: stale %d, expected %d", r.what, (int)stale(d), (int)r.stale);
    n_stale += r.stale;
    seen[r.source]++;
  }
  for (Source s : rest) {
    Changes c;
    c.happened(s);
    CHECK(!stale(c), "source %d alone: stale", (int)s);
    Changes d = neutral;
    d.happened(s);
    CHECK(!stale(d), "source %d with the neutral changes: stale", (int)s);
    seen[s]++;
  }
  bool once = true;
  for (int s = 0; s < kSourceCount; ++s) once = once && seen[s] == 1;
  CHECK(n_stale == 9 && sizeof(rows) / sizeof(rows[0]) == 22 && once, "the table lists every source (%d sources)", (int)kSourceCount);
  // the sampling rate and the clip box: only a changed value
  for (Source s : { kSamplingRate, kClipBox, kLightDirection, kShadowCell, kShadowMode }) {
    Changes c;
    c.note(s, true, false);
    CHECK(!stale(c), "source %d set to the same value: stale", (int)s);
  }
  // ... the grid convention and the transfer function: any call
  for (Source s : { kGridConvention, kTransferFunction }) {
    Changes c;
    c.note(s, true, false);
    CHECK(stale(c), "source %d set to the same value: not stale", (int)s);
  }
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "single_new", single_new }, { "single_same", single_same }, { "nothing_set", nothing_set }, { "pending_reset", pending_reset },
                                       { "camera_class", camera_class }, { "void_rule", void_rule }, { "sweep", sweep }, { "shadow_staleness", shadow_staleness } };

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
