// commit_plan.hpp - what a changed parameter invalidates, stated once.  ovr_hip_commit (and the four calls that change the scene without a commit: the
// volume upload, ovr_hip_update_volume, the noise tile, the supplied shadow values) record WHAT HAPPENED as `Changes`; plan_commit turns them into
// `Effects` - WHAT MUST HAPPEN - by the table below; apply_effects (volume.cpp) carries the effects out and is the only code that does.  Nothing here calls
// HIP or knows the renderer: tests/commit_plan_driver.cpp holds the table to literals on a machine without a GPU, like policy.hpp and launch_plan.hpp.
#pragma once

namespace ovrhip {
namespace commit {

// ---- what happened.  Per source: `set` - its setter was called since the last commit (Queued::update() returned true; for an event: it happened) - and
// `differs` - the committed value is not, byte for byte, the one before.  Where the rules distinguish parts of one setter's value, each part is a source.
enum Source : int {
  // the queued values, in the order ovr_hip_commit consumes them
  kFramebuffer, kCamera, kTransferFunction, kGridConvention, kFocus, kSpp, kSparse, kAccumulation, kSamplingRate, kShading, kJitter,
  kConvergence,          // differs: the MODE differs (a new threshold alone is a call with the same mode)
  kReconstruction,       // differs: the mode differs
  kLightVector,          // ovr_hip_set_light's vector as given
  kLightDirection,       // ... normalised: the unit vector the shadow march runs along (differs less often: a longer vector, the same direction)
  kLightIntensity,
  kMaterial, kClipBox,
  kShadowMode, kShadowCell, // ovr_hip_set_shadow_cache
  kShadowLeavesSupplied,    // differs: the mode differs and was SUPPLIED
  kShadowEntersMarched,     // differs: the mode differs and is MARCHED now
  kLdsStaging, kLayoutChoice, kPipeline, kSkipping, kShard,
  // the events that are no commit
  kVolumeUpload,   // ovr_hip_set_volume
  kVolumeUpdate,   // ovr_hip_update_volume
  kNoiseTile,      // ovr_hip_set_noise_tile
  kShadowValues,   // ovr_hip_set_shadow_cache_values; differs: the committed mode is SUPPLIED - a frame reads them
  kSourceCount
};

struct Changes {
  struct One { bool set = false, differs = false; };
  One of[kSourceCount];
  void note(Source s, bool set, bool differs) { of[s].set = set; of[s].differs = set && differs; }
  void happened(Source s) { note(s, true, true); }
};

// ---- what must happen
enum Effect : unsigned {
  kReset = 1u << 0,               // the accumulation starts over (ovr_hip_renderer::fb_reset)
  kResort = 1u << 1,              // the schedule is sorted again (ScheduleState::dirty)
  kRelist = 1u << 2,              // the list of owned blocks is rebuilt (ScheduleState::list_dirty)
  kBumpClearGen = 1u << 3,        // what the pixels of the blocks that are not launched hold is void (ScheduleState::clear_gen)
  kPoolUnproven = 1u << 4,        // the next frame's request count is unknown (ovr_hip_renderer::pool_roomy)
  kMajorantVoid = 1u << 5,        // the macrocells' majorants (and with them the adaptive-skipping probe, policy::Skip::before_frame)
  kRangesVoid = 1u << 6,          // the macrocells' value ranges
  kSkipRestart = 1u << 7,         // policy::Skip::restart
  kLatticeStale = 1u << 8,        // the built shadow lattice (ShadowCacheState::built_valid)
  kEstimateVoid = 1u << 9,        // the convergence estimate, the retired blocks (ConvergenceState)
  // buffers a mode no longer needs.  Freeing can fail, so the commit carries these four out itself, where it consumes the value (effects_of)
  kFreeConvergence = 1u << 10, kFreeReconstruction = 1u << 11, kFreeSuppliedLattice = 1u << 12, kFreeBuiltLattice = 1u << 13,
  // frame parameters derived again from the committed values
  kCameraParams = 1u << 14,       // update_camera - only with a framebuffer (CommitFacts::framebuffer): without one the camera stays dirty
  kVolumeParams = 1u << 15,       // update_volume_params - only with a volume (CommitFacts::volume)
  kLighting = 1u << 16,           // apply_lighting
  kClipParams = 1u << 17,         // apply_clip_box
};
// what a commit does for every change that shapes the frame.  (The volume calls and the noise tile do less: their rows spell out what.)
constexpr unsigned kChanged = kReset | kBumpClearGen | kPoolUnproven | kEstimateVoid;

// what becomes of the layout / pipeline tuner's measurement (policy::Tuner), weakest first
enum Tuner : int {
  kTunerKeeps = 0,
  kTunerCameraMoved,     // configuration_changed(true): a measured decision outlives camera moves
  kTunerStateZero,       // state = 0, as the volume calls write it (Tuner::recheck stays)
  kTunerChanged,         // configuration_changed(false)
  kTunerVoid,            // restart(): measured under another layout choice, pipeline or shadow mode
};

struct Effects {
  unsigned what = 0;
  Tuner tuner = kTunerKeeps;
  bool has(Effect e) const { return (what & e) != 0; }
};

// what plan_commit reads besides the changes
struct CommitFacts {
  bool reset_pending = false; // a commit: a reset it found pending (or its own failure half-way through).  The other calls leave a pending reset as it is
  bool camera_dirty = false;  // the camera's parameters were never derived (no framebuffer yet): counts as a camera that was set
  bool framebuffer = false;   // the committed framebuffer is not empty
  bool volume = false;        // a volume is resident
};

enum Trigger : int { kOnSet, kOnDiffers };
struct Row { Source source; Trigger when; unsigned effects; Tuner tuner; };

// ---- the table: per source, when its row fires and what follows.  A source without an effect has a row that says so.
constexpr Row kRows[] = {
  // a new framebuffer (resize_framebuffers has relisted the blocks) is seen through a new camera; to the tuner it is not a camera move
  { kFramebuffer, kOnSet, kChanged | kResort | kCameraParams, kTunerChanged },
  { kCamera, kOnSet, kChanged | kResort | kCameraParams, kTunerCameraMoved },
  { kTransferFunction, kOnSet, kChanged | kMajorantVoid | kLatticeStale, kTunerChanged },
  { kGridConvention, kOnSet, kChanged | kResort | kVolumeParams | kLatticeStale, kTunerChanged },
  { kFocus, kOnSet, kChanged, kTunerChanged },
  { kSpp, kOnSet, kChanged | kResort, kTunerChanged }, // (one sample per pixel: the schedule knows every ray)
  { kSparse, kOnSet, kChanged, kTunerChanged },
  { kAccumulation, kOnSet, kChanged, kTunerChanged },
  { kSamplingRate, kOnSet, kChanged, kTunerChanged },
  { kSamplingRate, kOnDiffers, kLatticeStale, kTunerKeeps },
  // (the frame kinds - ovr_hip_set_projection, ovr_hip_set_isosurfaces, ovr_hip_set_ambient_occlusion, ovr_hip_set_slices, ovr_hip_set_slice_context, ovr_hip_set_isosurface_context, ovr_hip_set_preintegration, ovr_hip_set_gradient_opacity, ovr_hip_set_max_depth, ovr_hip_set_depth_output - are recorded under kShading: any call
  // starts the accumulation over, and voids nothing else - no majorant, range, lattice, schedule or block list depends on which kernel draws the frame)
  { kShading, kOnSet, kChanged, kTunerChanged },
  { kJitter, kOnSet, kChanged | kResort, kTunerChanged },
  { kConvergence, kOnSet, kChanged, kTunerChanged },       // any call: retired blocks come back, the estimate starts over
  { kConvergence, kOnDiffers, kFreeConvergence, kTunerKeeps }, // OFF keeps no buffer; the other two allocate what they need with their next frame
  { kReconstruction, kOnSet, kChanged, kTunerChanged },
  { kReconstruction, kOnDiffers, kFreeReconstruction, kTunerKeeps }, // OFF keeps no buffer; FILL allocates with its next sparse frame
  // light, material, clip box, shadow cache: the same value again changes nothing
  { kLightVector, kOnSet, kLighting, kTunerKeeps },
  { kLightVector, kOnDiffers, kChanged, kTunerChanged },   // shadow rays change their length with the light
  { kLightDirection, kOnDiffers, kLatticeStale, kTunerKeeps },
  { kLightIntensity, kOnDiffers, kChanged, kTunerChanged },
  { kMaterial, kOnSet, kLighting, kTunerKeeps },
  { kMaterial, kOnDiffers, kChanged, kTunerChanged },
  { kClipBox, kOnSet, kClipParams, kTunerKeeps },
  { kClipBox, kOnDiffers, kChanged | kResort | kLatticeStale, kTunerChanged }, // the schedule's block test is the clipped one; a cut volume is another workload
  { kShadowMode, kOnDiffers, kChanged | kLatticeStale, kTunerVoid },        // another shadow term; a cached frame is another workload
  { kShadowCell, kOnDiffers, kChanged | kLatticeStale, kTunerChanged },
  { kShadowLeavesSupplied, kOnDiffers, kFreeSuppliedLattice, kTunerKeeps }, // the caller's values are kept until the mode leaves SUPPLIED
  { kShadowEntersMarched, kOnDiffers, kFreeBuiltLattice, kTunerKeeps },     // MARCHED keeps no buffer
  // every layout, both pipelines, skipping or not, LDS staging or not give the same frame bit for bit: no reset
  { kLdsStaging, kOnSet, 0, kTunerKeeps },
  { kLayoutChoice, kOnDiffers, 0, kTunerVoid }, // a probe must not override a layout forced meanwhile; forced -> automatic has to measure again
  { kPipeline, kOnDiffers, 0, kTunerVoid },
  { kSkipping, kOnSet, kSkipRestart, kTunerKeeps },
  { kShard, kOnSet, kChanged | kRelist, kTunerChanged },
  // The calls that are no commit.  Kept as found: the upload does not void the estimate where the update does; both write the
  // tuner's state = 0 where a commit restarts it; neither bumps the clear generation
  { kVolumeUpload, kOnSet, kReset | kResort | kPoolUnproven | kRangesVoid | kMajorantVoid | kLatticeStale | kVolumeParams, kTunerStateZero },
  { kVolumeUpdate, kOnSet, kReset | kEstimateVoid | kPoolUnproven | kMajorantVoid | kLatticeStale, kTunerStateZero }, // (the lattice: a whole rebuild)
  { kNoiseTile, kOnSet, kReset, kTunerKeeps },
  { kShadowValues, kOnDiffers, kReset, kTunerKeeps }, // another shadow term: the accumulation starts over
};

inline bool fires(const Row& row, const Changes& c) { return row.when == kOnSet ? c.of[row.source].set : c.of[row.source].differs; }

// the effects of one source's rows that fire: what the commit asks where it consumes a value whose buffers it may have to free
inline unsigned effects_of(const Changes& c, Source s)
{
  unsigned what = 0;
  for (const Row& row : kRows)
    if (row.source == s && fires(row, c)) what |= row.effects;
  return what;
}

// The combiner.  Every effect is the OR over the rows that fired: no row takes back what another asked for.  The tuner's fate is the one exception, and
// it is the strongest of the fired rows' columns in the order of `Tuner`: void if any row voids the measurement; else "changed" if anything outside the
// camera class fired; else (state = 0 if a volume call fired; else) "the camera moved" if only the camera class did; else nothing.  A pending reset adds
// what a commit does with it; the two derivations that need a framebuffer or a volume are dropped without one.
inline Effects plan_commit(const Changes& changes, const CommitFacts& facts)
{
  Changes c = changes;
  if (facts.camera_dirty) c.of[kCamera].set = true;
  Effects e;
  for (const Row& row : kRows)
    if (fires(row, c)) {
      e.what |= row.effects;
      if (row.tuner > e.tuner) e.tuner = row.tuner;
    }
  if (facts.reset_pending) e.what |= kReset | kEstimateVoid;
  if (!facts.framebuffer) e.what &= ~(unsigned)kCameraParams;
  if (!facts.volume) e.what &= ~(unsigned)kVolumeParams;
  return e;
}

} // namespace commit
} // namespace ovrhip
