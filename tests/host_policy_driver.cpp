// Driver of tests/test_host_policy.py: runs csrc/host/policy.hpp - the host state machine's automatic decisions - through scripted frame
// sequences on the CPU.  `driver <scenario>` exits 0 when every frame of the scenario did what its table row expects; the expectations are the
// rules as DESIGN.md sections 2 / 4 and the comments in policy.hpp state them.  The frame loop below does what frame.cpp does around the policies.
#include "policy.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace ovrhip::policy;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } \
  } while (0)

// ---- work of a frame: every sample shaded with 3 shadow taps (shade-heavy), 60 % shaded without shadows (not shade-heavy, but >= 50 % shaded: the
// automatic pipeline goes in place), 10 % shaded (not shade-heavy, < 35 %: pooled)
enum Work { HEAVY, HALF, LIGHT };
static FrameWork work(Work k)
{
  FrameWork w;
  w.shading = 1; w.spp = 1; w.samples = 1000;
  w.shaded_samples = k == HEAVY ? 1000 : k == HALF ? 600 : 100;
  w.shadow_samples = k == HEAVY ? 3000 : 0;
  return w;
}

enum Event { NONE, BUILT, CAMERA_MOVED }; // before the frame: every replica under construction becomes resident / a commit that changed the camera alone
struct Frame {
  Event ev; int rule; Work work; float ms; // the script: rule = what the layout rule says for this frame's camera
  int layout, pipeline, timed;             // expected: the layout and pipeline (1 in place, 2 pooled) the frame renders, is it a candidate's frame
};

struct Session {
  Tuner t; AutoPipeline ap;
  int states[kLayoutCount] = { kReplicaResident, kReplicaNone, kReplicaNone, kReplicaNone };
  bool free_layout = true, free_pipeline = true;
  int pipe_setting() const { return free_pipeline ? 0 : 2; }
  void run(const char* name, const std::vector<Frame>& frames)
  {
    for (size_t i = 0; i < frames.size(); ++i) {
      const Frame& f = frames[i];
      if (f.ev == BUILT) for (int& s : states) if (s == kReplicaClaimed || s == kReplicaEnqueued) s = kReplicaResident;
      if (f.ev == CAMERA_MOVED) t.configuration_changed(true);
      int rule = f.rule;
      if (states[rule] == kReplicaNone) rule = kGeneral;
      bool building = false;
      if (t.on && (free_layout || free_pipeline) && t.state == 1) {
        const int wanted = t.probe_build(free_layout, states);
        if (wanted >= 0) states[wanted] = kReplicaClaimed;
        for (int s : states) building = building || s == kReplicaClaimed || s == kReplicaEnqueued;
      }
      const int choice = t.before_frame(rule, free_layout, free_pipeline, building);
      const int layout = states[choice] == kReplicaResident ? choice : kGeneral; // (resolve_layout)
      const int pipeline = ap.want_pool(1, pipe_setting(), t.measured_pipeline()) ? 2 : 1;
      CHECK(layout == f.layout, "%s frame %zu: layout %d, expected %d", name, i + 1, layout, f.layout);
      CHECK(pipeline == f.pipeline, "%s frame %zu: pipeline %d, expected %d", name, i + 1, pipeline, f.pipeline);
      CHECK((t.frame >= 0) == (f.timed != 0), "%s frame %zu: candidate %d, expected %d", name, i + 1, t.frame, f.timed);
      FrameWork w = work(f.work);
      w.layout = layout; w.pipeline = pipeline; w.kernel_ms = f.ms;
      const Tuner::After a = t.after_frame(w, free_layout, free_pipeline, states);
      for (int k = 1; k < kLayoutCount; ++k)
        if (a.builds & (1u << k)) { CHECK(states[k] == kReplicaPlanned, "%s frame %zu: build of replica %d", name, i + 1, k); states[k] = kReplicaClaimed; }
      ap.after_frame(w);
      CHECK(t.n <= 6, "%s frame %zu: %d candidates", name, i + 1, t.n);
    }
  }
};

// ---- layout rule: a dominant direction component >= 0.93 picks the thin replica whose pair axis is not that axis; along z the tie goes by ax >= ay
static void layout_rule_cases()
{
  struct { float d[3]; int want; } cases[] = {
    { { 1.f, 0.f, 0.f }, kThinT }, { { 0.f, -1.f, 0.f }, kThin },
    { { 0.94f, 0.3f, 0.16f }, kThinT }, { { 0.3f, 0.94f, 0.16f }, kThin },          // |d| = 1.0: the components are the normalised ones
    { { 0.2f, 0.1f, 0.97f }, kThinT }, { { 0.1f, 0.2f, 0.97f }, kThin }, { { 0.f, 0.f, 1.f }, kThinT }, // along z: ax >= ay
    { { 0.92f, 0.39f, 0.f }, kGeneral }, { { 0.39f, 0.92f, 0.f }, kGeneral }, { { 0.39f, 0.f, 0.92f }, kGeneral }, // 0.92 (|d| = 0.9992): general
    { { 0.577f, 0.577f, 0.577f }, kGeneral },
  };
  const float unit[3] = { 1.f, 1.f, 1.f };
  for (const auto& c : cases) CHECK(layout_rule(c.d, unit) == c.want, "dir %g %g %g", c.d[0], c.d[1], c.d[2]);
  // the direction is taken in object space: a volume 4x as long in x (inv_scale.x = 1/4) turns a 0.94-in-x view into an oblique one
  const float d[3] = { 0.94f, 0.3f, 0.16f }, squeezed[3] = { 0.25f, 1.f, 1.f };
  CHECK(layout_rule(d, squeezed) == kGeneral, "object space");
}

// ---- tuner
// a first frame that is not shade-heavy decides at once, for the rules
static void tuner_light()
{
  Session s; s.states[kQuad] = kReplicaPlanned;
  s.run("tuner_light", { { NONE, kGeneral, LIGHT, 3.f, kGeneral, 2, 1 }, { NONE, kGeneral, LIGHT, 3.f, kGeneral, 2, 0 }, { NONE, kGeneral, LIGHT, 3.f, kGeneral, 2, 0 } });
  CHECK(s.t.state == 2 && s.t.layout == -1 && s.t.pipeline == 0 && s.t.status() == 0 && s.states[kQuad] == kReplicaPlanned, "the rules stay in charge");
}

// shade-heavy, pipelines within a quarter of each other (pooled 10, in place 9): two frames per candidate, the second one timed; then the quad
// replica under both pipelines (general is the rules' layout); nothing counts while the replica is being built; the fastest timed candidate wins.
// The first (untimed) frames carry times that would win if they counted.
static void tuner_heavy_close()
{
  Session s; s.states[kQuad] = kReplicaPlanned;
  s.run("tuner_heavy_close", {
    { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 2, 1 },  // the rules' frame: general, pooled (nothing measured, auto pipeline starts pooled)
    { NONE, kGeneral, HEAVY, 10.f, kGeneral, 2, 1 },  // ... once more, timed
    { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 1, 1 },  // the other pipeline
    { NONE, kGeneral, HEAVY, 9.f, kGeneral, 1, 1 },   // ... timed: in place is better, within a quarter -> quad in place, quad pooled; the build starts
    { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 2, 0 },  // building: the rules' choice (and the pipeline their frame ran), counts for nothing
    { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 2, 0 },
    { BUILT, kGeneral, HEAVY, 0.1f, kQuad, 1, 1 },
    { NONE, kGeneral, HEAVY, 7.f, kQuad, 1, 1 },
    { NONE, kGeneral, HEAVY, 0.1f, kQuad, 2, 1 },
    { NONE, kGeneral, HEAVY, 6.f, kQuad, 2, 1 },      // decided: quad, pooled (6 ms)
    { NONE, kGeneral, HEAVY, 6.f, kQuad, 2, 0 },
    { NONE, kGeneral, HEAVY, 6.f, kQuad, 2, 0 },
  });
  CHECK(s.t.state == 2 && s.t.layout == kQuad && s.t.pipeline == 2 && s.t.n == 4 && s.t.status() == 2, "decision: state %d layout %d pipeline %d n %d", s.t.state, s.t.layout, s.t.pipeline, s.t.n);
}

// shade-heavy, in place twice as fast as pooled: the layouts are tried under in place only; the rules' thin replica stays the fastest.
// The rules' layout is a thin replica here, so general is a candidate too
static void tuner_heavy_apart()
{
  Session s; s.states[kThin] = s.states[kThinT] = kReplicaResident; s.states[kQuad] = kReplicaResident;
  s.run("tuner_heavy_apart", {
    { NONE, kThinT, HEAVY, 0.1f, kThinT, 2, 1 }, { NONE, kThinT, HEAVY, 10.f, kThinT, 2, 1 },
    { NONE, kThinT, HEAVY, 0.1f, kThinT, 1, 1 }, { NONE, kThinT, HEAVY, 5.f, kThinT, 1, 1 },
    { NONE, kThinT, HEAVY, 0.1f, kGeneral, 1, 1 }, { NONE, kThinT, HEAVY, 8.f, kGeneral, 1, 1 },
    { NONE, kThinT, HEAVY, 0.1f, kQuad, 1, 1 }, { NONE, kThinT, HEAVY, 6.f, kQuad, 1, 1 },
    { NONE, kThinT, HEAVY, 5.f, kThinT, 1, 0 },
  });
  CHECK(s.t.state == 2 && s.t.layout == kThinT && s.t.pipeline == 1 && s.t.n == 4, "decision: state %d layout %d pipeline %d n %d", s.t.state, s.t.layout, s.t.pipeline, s.t.n);
}

// no replica exists: the pipelines are all there is to try
static void tuner_no_replicas()
{
  Session s;
  s.run("tuner_no_replicas", { { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 2, 1 }, { NONE, kGeneral, HEAVY, 4.f, kGeneral, 2, 1 }, { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 1, 1 },
                               { NONE, kGeneral, HEAVY, 5.f, kGeneral, 1, 1 }, { NONE, kGeneral, HEAVY, 4.f, kGeneral, 2, 0 } });
  CHECK(s.t.state == 2 && s.t.pipeline == 2 && s.t.n == 2, "decision: state %d pipeline %d n %d", s.t.state, s.t.pipeline, s.t.n);
}

// a forced layout is never overridden: only the pipelines are probed, every frame reads the forced layout
static void tuner_forced_layout()
{
  Session s; s.free_layout = false; s.states[kThin] = kReplicaResident; s.states[kQuad] = kReplicaResident;
  s.run("tuner_forced_layout", { { NONE, kThin, HEAVY, 0.1f, kThin, 2, 1 }, { NONE, kThin, HEAVY, 10.f, kThin, 2, 1 }, { NONE, kThin, HEAVY, 0.1f, kThin, 1, 1 },
                                 { NONE, kThin, HEAVY, 9.f, kThin, 1, 1 }, { NONE, kThin, HEAVY, 9.f, kThin, 1, 0 }, { NONE, kThin, HEAVY, 9.f, kThin, 1, 0 } });
  CHECK(s.t.state == 2 && s.t.layout == -1 && s.t.pipeline == 1, "decision: state %d layout %d pipeline %d", s.t.state, s.t.layout, s.t.pipeline);
}

// a decision kept across camera moves: the measured layout holds while the rule says what it said, the measured pipeline holds anyway; a frame
// that is not shade-heavy gives both back to the rules
static void tuner_kept_decision()
{
  Session s; s.states[kThin] = s.states[kThinT] = s.states[kQuad] = kReplicaResident;
  s.run("tuner_kept_decision", {
    { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 2, 1 }, { NONE, kGeneral, HEAVY, 10.f, kGeneral, 2, 1 }, { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 1, 1 }, { NONE, kGeneral, HEAVY, 20.f, kGeneral, 1, 1 },
    { NONE, kGeneral, HEAVY, 0.1f, kQuad, 2, 1 }, { NONE, kGeneral, HEAVY, 6.f, kQuad, 2, 1 },  // decided: quad, pooled
    { CAMERA_MOVED, kGeneral, HEAVY, 6.f, kQuad, 2, 0 },   // the rule still says general: the measured layout stays
    { CAMERA_MOVED, kThinT, HEAVY, 6.f, kThinT, 2, 0 },    // the rule says something else: its choice, under the measured pipeline (the rules alone
    { CAMERA_MOVED, kGeneral, HEAVY, 6.f, kGeneral, 2, 0 }, //   would shade in place: every sample is shaded); the measured layout does not come back
    { CAMERA_MOVED, kGeneral, HALF, 6.f, kGeneral, 2, 0 }, // not shade-heavy any more ...
    { CAMERA_MOVED, kGeneral, HALF, 6.f, kGeneral, 1, 1 }, // ... back to the rules (in place: >= 50 % shaded), and - the camera keeps moving - a new measurement starts
  });
}

// ... and it is measured again once the configuration has been static for a while (12 frames after the last camera move)
static void tuner_recheck()
{
  Session s; s.states[kQuad] = kReplicaResident;
  std::vector<Frame> f = { { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 2, 1 }, { NONE, kGeneral, HEAVY, 10.f, kGeneral, 2, 1 }, { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 1, 1 },
                           { NONE, kGeneral, HEAVY, 20.f, kGeneral, 1, 1 }, { NONE, kGeneral, HEAVY, 0.1f, kQuad, 2, 1 }, { NONE, kGeneral, HEAVY, 6.f, kQuad, 2, 1 } };
  f.push_back({ CAMERA_MOVED, kGeneral, HEAVY, 6.f, kQuad, 2, 0 });
  for (int i = 0; i < 11; ++i) f.push_back({ NONE, kGeneral, HEAVY, 6.f, kQuad, 2, 0 });
  f.push_back({ NONE, kGeneral, HEAVY, 6.f, kGeneral, 1, 1 }); // the 13th frame: the first of a new measurement, the rules' choice (in place: every sample shaded)
  s.run("tuner_recheck", f);
  CHECK(s.t.state == 1, "probing again: state %d", s.t.state);
}

// a commit that changes more than the camera voids the measurement; OVR_HIP_TUNE=0 (on = false) keeps the rules alone
static void tuner_reset_and_off()
{
  Session s;
  s.run("tuner_reset", { { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 2, 1 }, { NONE, kGeneral, HEAVY, 4.f, kGeneral, 2, 1 }, { NONE, kGeneral, HEAVY, 0.1f, kGeneral, 1, 1 },
                         { NONE, kGeneral, HEAVY, 5.f, kGeneral, 1, 1 } });
  s.t.configuration_changed(false);
  CHECK(s.t.state == 0 && s.t.recheck == 0, "reset");
  Session off; off.t.on = false; off.states[kQuad] = kReplicaResident;
  off.run("tuner_off", { { NONE, kGeneral, HEAVY, 1.f, kGeneral, 2, 0 }, { NONE, kGeneral, HEAVY, 1.f, kGeneral, 1, 0 }, { NONE, kGeneral, HEAVY, 1.f, kGeneral, 1, 0 } });
}

// ---- automatic pipeline: >= 50 % of the steps shaded and no long shadows -> in place; < 35 %, or more than 60 shadow iterations per shaded
// sample -> pooled; in between the setting is kept.  Steps are the samples taken and the samples skipped
static void auto_pipeline()
{
  struct { uint64_t samples, skipped, shaded, shadow; int want; } rows[] = { // want: 1 in place, 0 pooled
    { 1000, 0, 500, 0, 1 }, { 1000, 0, 499, 0, 1 }, { 1000, 0, 351, 0, 1 }, { 1000, 0, 349, 0, 0 }, { 1000, 0, 499, 0, 0 }, { 1000, 0, 351, 0, 0 },
    { 600, 400, 500, 0, 1 }, { 600, 400, 349, 0, 0 },           // skipped steps count
    { 1000, 0, 900, 900 * 60, 1 }, { 1000, 0, 900, 900 * 60 + 1, 0 }, // long shadows
    { 1000, 0, 400, 400 * 60 + 1, 0 }, { 1000, 0, 500, 0, 1 }, { 1000, 0, 400, 400 * 60 + 1, 0 }, // ... also from the band in between
    { 0, 0, 0, 0, 0 },                                          // an empty frame says nothing
  };
  AutoPipeline ap;
  CHECK(!ap.inplace && ap.want_pool(1, 0, 0) && !ap.want_pool(0, 0, 0) && !ap.want_pool(1, 1, 0) && ap.want_pool(1, 2, 0), "pooled at first; unshaded frames have no pool");
  int i = 0;
  for (const auto& r : rows) {
    FrameWork w; w.shading = 1; w.samples = r.samples; w.skipped_samples = r.skipped; w.shaded_samples = r.shaded; w.shadow_samples = r.shadow;
    ap.after_frame(w);
    CHECK(ap.inplace == (r.want != 0), "row %d", i);
    CHECK(ap.want_pool(1, 0, 0) == !ap.inplace && ap.want_pool(1, 0, 1) == false && ap.want_pool(1, 0, 2) == true && ap.want_pool(1, 2, 1) == true, "row %d: a measured pipeline overrides the automatic one only", i);
    ++i;
  }
}

// ---- adaptive skipping.  frames(...) renders n frames whose skipped share of all steps is `percent` and returns the numbers of those that ran
// the skipping kernels
struct SkipSession {
  Skip s; int frame = 0;
  std::vector<int> frames(int n, int percent, bool majorant_valid = true)
  {
    std::vector<int> used;
    for (int i = 0; i < n; ++i) {
      ++frame;
      const bool use = s.before_frame(true, majorant_valid);
      majorant_valid = true; // (a frame that skips rebuilds the grid)
      if (use) used.push_back(frame);
      FrameWork w; w.samples = 600; w.shadow_samples = 400;
      if (use) { w.skipped_samples = (uint64_t)percent * 5; w.skipped_shadow_samples = (uint64_t)percent * 5; w.samples -= w.skipped_samples; w.shadow_samples -= w.skipped_shadow_samples; }
      s.after_frame(w);
    }
    return used;
  }
};
static void skipping()
{
  { // skipping < 10 % of the steps switches it off; re-probes come after 32, 64, 128, 256, 256 ... frames
    SkipSession k;
    const std::vector<int> used = k.frames(1200, 9);
    const int want[] = { 1, 33, 97, 225, 481, 737, 993 };
    CHECK(used.size() == 7, "%zu probes", used.size());
    for (size_t i = 0; i < used.size() && i < 7; ++i) CHECK(used[i] == want[i], "probe %zu at frame %d, expected %d", i, used[i], want[i]);
  }
  { // a frame that skipped >= 10 % keeps it on and resets the back-off to 32
    SkipSession k;
    k.frames(97 - 1, 9);                              // probes at 1, 33 failed: the next one at 97, the one after it 128 frames later
    std::vector<int> used = k.frames(10, 11);         // frames 97 .. 106: the probe pays, so does every frame after it
    CHECK(used.size() == 10 && used[0] == 97, "%zu frames skipped", used.size());
    used = k.frames(40, 9);                           // frame 107 does not pay: off, and back 32 frames later
    CHECK(used.size() == 2 && used[0] == 107 && used[1] == 139, "%zu probes", used.size());
  }
  { // an invalid majorant grid (new transfer function / volume) switches it on at once and resets the back-off to 32
    SkipSession k;
    k.frames(50, 9);                                  // off since frame 33, next probe at 97
    std::vector<int> used = k.frames(1, 9, false);
    CHECK(used.size() == 1 && used[0] == 51, "on at once");
    used = k.frames(40, 9);
    CHECK(used.size() == 1 && used[0] == 83, "back-off 32: %zu probes", used.size());
  }
  { // OVR_HIP_SKIP_ADAPTIVE=0 keeps the skipping kernels whatever they skip; skipping disabled never uses them
    SkipSession k; k.s.adaptive = false;
    CHECK(k.frames(100, 0).size() == 100, "not adaptive");
    Skip off;
    CHECK(!off.before_frame(false, true) && !off.frame_used, "disabled");
  }
}

// ---- the small rules
static void small_rules()
{
  CHECK(schedule_exact(true, false, 1, 0) == 1 && schedule_exact(true, false, 2, 0) == 2 && schedule_exact(true, false, 1, 1) == 2, "exact / widened");
  CHECK(schedule_exact(false, false, 1, 0) == 0 && schedule_exact(true, true, 1, 0) == 0, "every block is launched");
  CHECK(shade_blocks(false, 1) == 768 && shade_blocks(false, 64 * 1024 * 4) == 768 && shade_blocks(false, 64 * 1024 * 4 + 1) == 1024, "few runs: 768 workgroups");
  CHECK(shade_blocks(false, 0) == 1024 && shade_blocks(true, 1000) == 1024, "no pooled frame yet / skipping: 1024");
  // 8 shaded samples per pixel in chunks of 64 requests, at least 4096 chunks, 4 more per tile, x 1.25, at most 2^22
  CHECK(pool_first_guess(1920 * 1080, 1000) == (size_t)(1920 * 1080 * 8 / 64 + 4000) * 5 / 4, "first guess");
  CHECK(pool_first_guess(64, 0) == 4096 * 5 / 4 && pool_first_guess((size_t)1 << 30, 0) == (size_t)1 << 22, "bounds of the first guess");
  CHECK(pool_grown(1000) == (1000 + 250 + 16) * 4, "+25 %% and a run, in every sub-pool");
}

int main(int argc, char** argv)
{
  struct { const char* name; void (*run)(); } scenarios[] = {
    { "layout_rule", layout_rule_cases }, { "tuner_light", tuner_light }, { "tuner_heavy_close", tuner_heavy_close }, { "tuner_heavy_apart", tuner_heavy_apart },
    { "tuner_no_replicas", tuner_no_replicas }, { "tuner_forced_layout", tuner_forced_layout }, { "tuner_kept_decision", tuner_kept_decision },
    { "tuner_recheck", tuner_recheck }, { "tuner_reset_and_off", tuner_reset_and_off }, { "auto_pipeline", auto_pipeline }, { "skipping", skipping },
    { "small_rules", small_rules },
  };
  if (argc == 2 && !strcmp(argv[1], "--list")) { for (const auto& s : scenarios) printf("%s\n", s.name); return 0; }
  for (const auto& s : scenarios)
    if (argc == 2 && !strcmp(argv[1], s.name)) { s.run(); printf("%s: %s\n", s.name, g_failed ? "FAILED" : "ok"); return g_failed ? 1 : 0; }
  fprintf(stderr, "usage: %s <scenario> | --list\n", argv[0]);
  return 2;
}
