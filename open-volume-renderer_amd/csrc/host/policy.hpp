// policy.hpp - the host state machine's automatic decisions as plain state and pure functions of a frame's counters: which layout of the volume
// a frame reads, which shading pipeline it runs, whether it uses the skipping kernels, how large the request pool is.  Nothing here calls HIP or
// knows the renderer: the callers (frame.cpp; volume.cpp's apply_effects for what a commit does to the tuner and the skip probe) carry out what a policy
// returns - "start this replica's build", "render this layout" - and tests/test_host_policy.py drives the same code with scripted frames on a machine
// without a GPU.  What a changed parameter invalidates is not a policy of a frame's counters: commit_plan.hpp states it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace ovrhip {
namespace policy {

// ovr_hip_kernels.h's VolumeLayout / kLayouts / kPoolSubs, restated (that header needs the HIP runtime); frame.cpp asserts that they agree
enum : int { kGeneral = 0, kThin = 1, kThinT = 2, kQuad = 3 };
constexpr int kLayoutCount = 4;
constexpr int kPoolSubCount = 4;

// build states of a replica (ovr_hip_renderer::replica_state)
enum : int { kReplicaNone = 0, kReplicaPlanned = 1, kReplicaEnqueued = 2, kReplicaResident = 3, kReplicaClaimed = 4 };

// which replica of the volume a frame reads (ovr_hip_kernels.h "View-dependent replicas"): the central ray's direction in
// object space; within ~21 degrees of an axis (measured crossover 18-23 degrees, profiles/r02_notes.md) a thin replica
inline int layout_rule(const float dir[3], const float inv_scale[3])
{
  const float dx = dir[0] * inv_scale[0], dy = dir[1] * inv_scale[1], dz = dir[2] * inv_scale[2];
  const float len = std::sqrt(dx * dx + dy * dy + dz * dz);
  const float ax = std::fabs(dx) / len, ay = std::fabs(dy) / len, az = std::fabs(dz) / len;
  // rays along x need the replica that is thin in y (pair axis y), rays along y the one thin in x; rays along z can use
  // either - the one that is 4 voxels wide in the direction the rays drift to is 4-7 % faster (profiles/r02_notes.md)
  int choice = kGeneral;
  const float kAxis = 0.93f; // ~21 degrees
  if (ax >= kAxis) choice = kThinT;
  else if (ay >= kAxis) choice = kThin;
  else if (az >= kAxis) choice = ax >= ay ? kThinT : kThin;
  return choice;
}

// what the policies read of a finished frame: its counters (ovr_hip_stats) and what it was launched with
struct FrameWork {
  uint64_t samples = 0, shaded_samples = 0, shadow_samples = 0, skipped_samples = 0, skipped_shadow_samples = 0;
  int shading = 0, spp = 1;     // RayMarchParams::shading / spp
  int layout = 0, pipeline = 0; // ovr_hip_stats::layout / pipeline: what the frame ran
  float kernel_ms = 0.f;        // first to last event
};

// shade-heavy: the gradient (3 per shaded sample) and shadow taps outnumber the primary taps
inline bool shade_heavy(const FrameWork& w)
{
  const double shade_taps = 3.0 * (double)w.shaded_samples + (double)w.shadow_samples;
  return w.shading != 0 && w.samples > 0 && shade_taps >= 3.0 * (double)w.samples;
}

// Automatic choice of the volume layout and of the shading pipeline, second stage (round 3).  The rules of round 2 - thin replicas for
// axis views, in place once half the samples are shaded - were fitted on frames bound by HBM bytes.  Frames that shade (nearly) every
// sample - most of the reference's shipped scenes, every frame at the scene files' sampling rate 4 - are bound by the gather rate and
// the instruction stream instead, and what is fastest there depends on the volume's size, the view and the sampling rate in ways no
// rule captured (profiles/r03_notes.md: quad replica -7 ... -16 % on the big scenes, +25 % on C3 dense at rate 1; pooled 16 ms vs in place
// 24 ms on C3 front / dense at rate 4, the opposite at rate 1).  Every layout and both pipelines give the same frame bit for bit, so the
// renderer measures: the first frame of a configuration runs what the rules say; if its shading taps outnumber its primary taps, the
// following frames try the alternatives - first the other pipeline, then the other candidate layouts (general, quad) under the better
// pipeline - two frames each, the second one timed (the first one pages the replica in and sizes the request pool), and the fastest
// (hipEvent kernel time) is kept until the configuration changes.  OVR_HIP_TUNE=0 keeps the rules alone.
struct Tuner {
  struct Cand { int layout, pipeline, frames; float ms; };
  int state = 0;          // 0 = the next frame is the first of a configuration, 1 = probing, 2 = decided
  int phase = 0;          // probing: 0 = pipelines, 1 = layouts
  Cand cand[6] = {};
  int n = 0, cur = 0;
  int layout = -1, pipeline = 0; // decided (-1 / 0 = leave it to the rules)
  int rule_choice = -1;   // what the layout rule said for the camera the measurement was made with: a measured LAYOUT is only kept
                          // across camera moves while the rule still says the same (the thin replicas are view-dependent)
  int frame = -1;         // candidate index of the frame in flight, -1 = not a tuned frame
  bool on = true;
  // A camera that moves on every frame (the interactive app) never sits still long enough to be measured: when only the camera changed, a
  // measured decision is kept (the regime - transfer function, sampling rate, volume - is what decides, not the view), dropped as soon as a
  // frame is no longer shade-heavy, and measured again once the configuration has been static for `recheck` frames.
  int recheck = 0;

  // what was measured is void (a new volume, a layout or pipeline forced or freed meanwhile)
  void restart() { state = 0; recheck = 0; }
  // a commit changed something: `only_camera` = nothing but the camera
  void configuration_changed(bool only_camera)
  {
    const bool keep = on && only_camera && state == 2 && (layout >= 0 || pipeline != 0);
    if (keep) recheck = 12; // only the camera moved: the measured layout / pipeline stay (see recheck)
    else restart();         // ... and so are the fastest layout and pipeline
  }
  // the frames' amount of work changed under the probes (adaptive refinement retired blocks): candidates timed on different amounts of work
  // are not comparable - the tuner starts over
  void work_changed() { if (on && state == 1) state = 0; }

  // before a frame, while probing: the replica the candidate under test needs and that is only planned so far, or -1.  The caller starts its
  // build and then tells before_frame whether any replica is being built.
  int probe_build(bool free_layout, const int replica_state[kLayoutCount]) const
  {
    if (state != 1) return -1;
    const Cand& c = cand[cur];
    return (free_layout && c.layout > kGeneral && replica_state[c.layout] == kReplicaPlanned) ? c.layout : -1;
  }

  // before a frame: the layout it asks for.  rule_choice = what the layout rule (or a forced choice) says, free_layout / free_pipeline = whether
  // the layout / the pipeline is automatic, building = a replica is being built in the background.  Leaves `frame` (is this a timed candidate) and
  // `pipeline` (see measured_pipeline) for the rest of the frame.
  int before_frame(int rule, bool free_layout, bool free_pipeline, bool building)
  {
    int choice = rule;
    frame = -1;
    if (!(on && (free_layout || free_pipeline))) return choice;
    if (state == 0) { // the rules' candidate
      cand[0] = { free_layout ? choice : -1, 0, 0, 0.f };
      n = 1; cur = 0; phase = 0;
      layout = -1; pipeline = 0;
      frame = 0;
      rule_choice = rule;
    }
    else if (state == 1) {
      const Cand& c = cand[cur];
      // Nothing is probed while ANY replica is being built in the background: the frame runs the rules' choice and counts for nothing.
      // Waiting for the candidate's own replica on the device would stall an interactive frame for the length of the build (24 ms for
      // C3's 17 GB quad replica), and a candidate timed beside a build is timed wrong - the build has the memory system: the rules'
      // candidate measured 4.7 instead of 1.2 ms that way and lost to the quad replica it beats (profiles/r04_notes.md section 4)
      if (!building) {
        if (free_layout && c.layout >= 0) choice = c.layout; // (a forced layout is never overridden by a probe)
        pipeline = c.pipeline;
        frame = cur;
      }
      else pipeline = cand[0].pipeline; // the pipeline the rules' frame ran (cand[0] was filled in by its after_frame)
    }
    else if (layout >= 0 && free_layout) {
      // a measured layout outlives camera moves only while the layout rule still says what it said when the measurement was made:
      // the thin replicas are view-dependent (an axis view's winner loses 30-60 % at an oblique angle), and general / quad were
      // measured against THAT rule's choice.  The measured pipeline stays (the regime decides it, not the view).
      if (rule != rule_choice) layout = -1;
      else choice = layout; // (probed, hence resident)
    }
    return choice;
  }

  // the pipeline the frame runs instead of the rules' one while the pipeline is automatic: 0 = the rules', 1 = in place, 2 = pooled
  int measured_pipeline() const { return (on && state != 0) ? pipeline : 0; }
  // ovr_hip_stats::tuning of the frame in flight: 1 = a candidate, 2 = runs a measured decision, 0 = the rules
  int status() const
  {
    if (frame == 0 && state == 0) return 0; // the first frame of a configuration runs the rules' choice
    return frame >= 0 ? 1 : (on && state == 2 && (layout >= 0 || pipeline != 0)) ? 2 : 0;
  }

  struct After {
    unsigned builds = 0;   // bit k: replica k is wanted by a candidate to come - built while the candidates before it are timed
    bool decided = false;  // this frame ended the probing with a comparison: `layout` / `pipeline` hold the winner, timed best_ms
    float best_ms = 0.f;
  };
  // after a frame: w = what it did.  The replica states are read as they were when the frame was resolved.
  After after_frame(const FrameWork& w, bool free_layout, bool free_pipeline, const int replica_state[kLayoutCount])
  {
    After out;
    if (frame >= 0 && state < 2) { // measured choice of layout and pipeline
      Cand& c = cand[frame];
      c.frames++;
      c.ms = w.kernel_ms;
      auto decide = [&]() {
        int best = 0;
        for (int k = 1; k < n; ++k)
          if (cand[k].frames >= 2 && cand[k].ms < cand[best].ms) best = k;
        layout = free_layout ? cand[best].layout : -1;
        pipeline = free_pipeline ? cand[best].pipeline : 0;
        state = 2;
        out.decided = true;
        out.best_ms = cand[best].ms;
      };
      // the layouts worth a try besides the rules' one: the general layout and the quad replica (a thin replica the camera did not ask
      // for loses 30-60 %: profiles/r02_notes.md section 2)
      auto add_layouts = [&](int pipe) {
        const int base = cand[0].layout;
        for (int l : { (int)kGeneral, (int)kQuad })
          if (free_layout && l != base && (l == kGeneral || replica_state[l] != kReplicaNone) && n < 6) {
            cand[n++] = { l, pipe, 0, 0.f };
            if (replica_state[l] == kReplicaPlanned) out.builds |= 1u << l;
          }
        phase = 1;
      };
      if (state == 0) {
        c.layout = free_layout ? w.layout : -1;
        c.pipeline = w.pipeline;
        if (!shade_heavy(w)) { state = 2; layout = -1; pipeline = 0; } // the rules stay in charge
        else {
          state = 1;
          cur = 0;          // the rules' candidate runs once more, timed
          pipeline = c.pipeline;
          // the other pipeline: pooled is never far off, but shading in place is only worth a frame when most samples are shaded (with
          // few, a handful of waves shade alone for many milliseconds: DESIGN.md section 4)
          const bool try_other = free_pipeline && w.spp == 1 &&
                                 (c.pipeline == 1 || (double)w.shaded_samples >= 0.35 * ((double)w.samples + (double)w.skipped_samples));
          if (try_other) cand[n++] = { c.layout, c.pipeline == 2 ? 1 : 2, 0, 0.f };
          else add_layouts(c.pipeline);
          if (n == 1) decide();
        }
      }
      else if (c.frames >= 2) {
        cur++;
        if (cur >= n) {
          if (phase == 0) {
            const int pbest = (n > 1 && cand[1].ms < cand[0].ms) ? cand[1].pipeline : cand[0].pipeline;
            // the two pipelines within a quarter of each other on the rules' layout: the quad replica may order them the other way round (round 5: a 256 x 256 x 226
            // u16 volume, all samples shaded - general layout pooled 1.00 / in place 1.08 ms, quad replica pooled 0.89 / in place 0.77) - it gets both
            const bool close = n > 1 && std::min(cand[0].ms, cand[1].ms) * 1.25f >= std::max(cand[0].ms, cand[1].ms);
            const int pother = pbest == 2 ? 1 : 2;
            add_layouts(pbest);
            if (close && free_layout && free_pipeline && cand[0].layout != kQuad && replica_state[kQuad] != kReplicaNone && n < 6) cand[n++] = { kQuad, pother, 0, 0.f };
            if (cur >= n) decide();
          }
          else decide();
        }
      }
    }
    else if (on && frame < 0 && state == 2 && recheck > 0) { // a decision kept across camera moves
      if (!shade_heavy(w)) { layout = -1; pipeline = 0; recheck = 0; } // not that regime any more: back to the rules
      else if (--recheck == 0) state = 0;                              // static for a while: measure again
    }
    return out;
  }
};

// Shading pipeline in automatic mode (ovr_hip_set_shading_pipeline(0)): pooling the shading requests pays when few samples are
// shaded and they sit in few tiles (sparse transfer functions: 2.7 vs 3.4 ms on C3); when most samples are shaded every tile has
// the same work and the requests' round trip through HBM (32 B written, read, written and read again per sample) only costs -
// dense transfer functions 1.57 vs 1.99 ms, the shipped mechhand scene 3.9 vs 5.4 ms.  The renderer follows the previous frame:
// >= 50 % of its samples shaded -> in place, < 35 % -> pooled (both give the same frame bit for bit).
struct AutoPipeline {
  bool inplace = false;
  void after_frame(const FrameWork& w)
  {
    const double steps = (double)w.samples + (double)w.skipped_samples, shaded = (double)w.shaded_samples;
    if (steps > 0.0) {
      // (round 3) ... unless the shadow marches are long - more than 60 iterations per shaded sample, i.e. sampling rates above ~2 (the
      // stride is 10 / rate^2 voxels): then tiles differ again by what their shadow rays cross, and pooling wins by 30-50 % (C3 front /
      // dense at rate 4: 22.7 ms in place, 13.4 pooled; profiles/r03_notes.md section 5)
      const bool long_shadows = (double)w.shadow_samples > 60.0 * std::max(shaded, 1.0);
      if (shaded >= 0.50 * steps && !long_shadows) inplace = true;
      else if (shaded < 0.35 * steps || long_shadows) inplace = false;
    }
  }
  // pooled (march -> shade -> composite) when it applies, else in place.  pipe = ovr_hip_set_shading_pipeline's value (0 automatic, 1 in place,
  // 2 pooled), measured = Tuner::measured_pipeline()
  bool want_pool(int shading, int pipe, int measured) const
  {
    bool pool = shading != 0 && pipe != 1 && !(pipe == 0 && inplace);
    if (shading != 0 && pipe == 0 && measured != 0) pool = measured == 2; // measured (Tuner::state)
    return pool;
  }
};

// Empty-space skipping pays only where there is empty space: with nothing to skip its kernels cost 20-50 % more than the plain ones
// (dense transfer functions, a camera inside the data).  While skipping is enabled the renderer therefore watches what it skips: a
// frame that skipped < 10 % of its sample steps switches to the plain kernels (the frames are bit-identical either way) and the
// skipping kernels are probed again after 32, 64, ... 256 frames, or at once when the transfer function or the volume changes.
// OVR_HIP_SKIP_ADAPTIVE=0 keeps the skipping kernels whatever they skip (measurements).
struct Skip {
  bool adaptive = true, active = true, frame_used = false;
  int reprobe_in = 0, backoff = 32;

  void restart() { active = true; backoff = 32; }
  // before a frame: does it run the skipping kernels?  enabled = ovr_hip_set_empty_space_skipping, majorant_valid = the majorant grid is current
  bool before_frame(bool enabled, bool majorant_valid)
  {
    bool use_skip = enabled;
    if (use_skip && adaptive) {
      if (!majorant_valid) restart(); // new transfer function / volume: what is empty has changed
      else if (!active && --reprobe_in <= 0) active = true; // probe the skipping kernels again with this frame
      use_skip = active;
    }
    frame_used = use_skip;
    return use_skip;
  }
  void after_frame(const FrameWork& w)
  {
    if (!(frame_used && adaptive)) return;
    // did skipping pay?
    const double skipped = (double)w.skipped_samples + (double)w.skipped_shadow_samples;
    const double all = skipped + (double)w.samples + (double)w.shadow_samples;
    if (all > 0.0 && skipped < 0.10 * all) {
      active = false;
      reprobe_in = backoff;
      backoff = std::min(backoff * 2, 256);
    }
    else backoff = 32;
  }
};

// Request pool of the pooled pipeline, in chunks.  First guess: room for 8 shaded samples per pixel; grown after an overflow
// (every tile reserves runs of 8 chunks, so add one run per tile)
inline size_t pool_first_guess(size_t pixels, size_t pool_tiles)
{
  return std::min<size_t>((std::max<size_t>(pixels * 8 / 64, 4096) + pool_tiles * 4) * 5 / 4, (size_t)1 << 22); // x 1.25: sub-pools fill unevenly
}
// ... to what the frame needs (+25 %): asked = the most chunks any sub-pool was asked for in any generation of the frame
inline size_t pool_grown(size_t asked) { return (asked + asked / 4 + 16) * kPoolSubCount; }

// Shade grid: with at most 64 runs of 4 chunks per workgroup in the previous frame (sparse transfer functions; C3: 36 k runs) 768
// workgroups shade 4 % faster than 1024 - a smaller window of requests in flight, more of their bricks still in L2 - with many
// runs (dense transfer functions, 4K frames) 1024 hide more latency (profiles/r02_ab/r02b_ab_shadeblocks.txt).  Not with empty-space
// skipping - that shade kernel is bound by instructions, not by memory, and wants every wave: 0.67 vs 0.77 ms
inline int shade_blocks(bool use_skip, size_t prev_pool_chunks)
{
  return (!use_skip && prev_pool_chunks > 0 && prev_pool_chunks <= (size_t)64 * 1024 * 4) ? 768 : 1024;
}

// The shadow cache (ovr_hip_set_shadow_cache).  When a built lattice is stale is a column of commit_plan.hpp's table (kLatticeStale).
// nodes per axis of the lattice over dim voxels at a cell size >= 1: ceil(dim / cell) + 1
inline long long shadow_cache_nodes(int dim, int cell) { return ((long long)dim + cell - 1) / cell + 1; }
constexpr int kShadowCacheDefaultCell = 4; // a guess: unmeasured until tools/shadow_cache_bench.py has run

// a pixel's ray is known to the schedule kernels when it has one sample and no jitter: blocks without a hit are found exactly (1); with
// several samples or jitter its rays lie within half a pixel of the centre: blocks whose widened cone misses the box are found (2);
// 0 = every block is launched
inline int schedule_exact(bool skip_blocks, bool unsorted, int spp, int jitter_mode)
{
  return (!skip_blocks || unsorted) ? 0 : (spp == 1 && jitter_mode == 0) ? 1 : 2;
}

} // namespace policy
} // namespace ovrhip
