// ray_query.hpp - the seven known-answer ray queries (ovr_hip_project_floats ... ovr_hip_isosurface_ao_floats, include/ovr_hip.h) as data: one row per entry
// with everything in which the entries differ, and the two pure functions that read the rows.  Nothing here calls HIP: ray_query (ovr_hip_api.cpp) walks the
// one path of an entry by its row, launch_ray_query (ovr_hip_kernels.hip) launches the kernel twin of the row's frame kind - and tests/test_ray_query_table.py
// holds every row to the messages and sizes the entries had when each was written out by hand.
#pragma once

#include "launch_plan.hpp"

#include <cstddef>
#include <string>

namespace ovrhip {

constexpr int kQueryEinval = -1, kQueryEstate = -3; // include/ovr_hip.h OVR_HIP_EINVAL / OVR_HIP_ESTATE, restated (ovr_hip_api.cpp asserts that they agree)
constexpr int kQueryMaxEvents = 16;                 // of a record
constexpr int kQueryRotations = 16;                 // include/ovr_hip.h OVR_HIP_AO_ROTATIONS, likewise

enum class QueryNeeds { Nothing, Slices, Isovalues }; // what must be committed besides the volume
struct RayQuery {
  const char* name;                 // the entry, as its error messages spell it
  FrameKind kind;                   // the frame kind whose kernel twin it runs (kQuerySlice: the plane kernel's while every committed slice is a plane - query_runs)
  QueryNeeds needs;
  const char* setter;               // the setter its "nothing is committed" message names
  bool needs_context, needs_ao, needs_tf; // the context mode of `needs`, ambient-occlusion samples, a committed transfer function
  bool takes_range_skipping, takes_max_events, takes_rotation, takes_mode; // its arguments beyond (r, org, dir, out, n)
  int header_floats, event_floats;  // a ray's record: the header and what follows per event
  bool zeroed;                      // out is zeroed first: the kernel writes a ray's header and the events it met
  bool needs_preintegration = false; // pre-integration committed in mode SEGMENTS (trailing and defaulted: the seven rows below read as they did)
  bool needs_gradient_opacity = false, takes_shade = false; // gradient opacity committed in mode RAMP; `mode` is a shading mode, NONE (0) or GRADIENT (1) (likewise)
  bool takes_depth = false;         // one ray parameter per ray, a device pointer beside org and dir (likewise)
  bool takes_threshold = false, depth_optional = false; // the depth layer's tau in (0, 0.9999]; a null depth pointer means no limit on any ray (likewise)
};
enum RayQueryId { kQueryProject, kQuerySlice, kQuerySliceContext, kQueryIsosurface, kQueryIsosurfaceLayers, kQueryIsosurfaceContext, kQueryIsosurfaceAo, kRayQueryCount };
constexpr RayQuery kRayQueries[kRayQueryCount] = {
  // name                                 kind                          needs                  setter                           context ao     tf     skip   events rot    mode   record zeroed
  { "ovr_hip_project_floats",            FrameKind::Projection,        QueryNeeds::Nothing,   nullptr,                         false,  false, false, true,  false, false, true,  4, 0, false },
  { "ovr_hip_slice_floats",              FrameKind::SliceWalk,         QueryNeeds::Slices,    "ovr_hip_set_slices",            false,  false, false, true,  false, false, false, 4, 0, false },
  { "ovr_hip_slice_context_floats",      FrameKind::SliceContext,      QueryNeeds::Slices,    "ovr_hip_set_slices",            true,   false, true,  false, false, false, false, 8, 0, false },
  { "ovr_hip_isosurface_floats",         FrameKind::Isosurface,        QueryNeeds::Isovalues, "ovr_hip_set_isosurfaces",       false,  false, false, true,  false, false, false, 8, 0, false },
  { "ovr_hip_isosurface_layers_floats",  FrameKind::IsosurfaceLayers,  QueryNeeds::Isovalues, "ovr_hip_set_isosurface_layers", false,  false, false, true,  true,  false, false, 4, 8, true },
  { "ovr_hip_isosurface_context_floats", FrameKind::IsosurfaceContext, QueryNeeds::Isovalues, "ovr_hip_set_isosurfaces",       true,   false, true,  false, true,  false, false, 8, 8, true },
  { "ovr_hip_isosurface_ao_floats",      FrameKind::IsosurfaceAo,      QueryNeeds::Isovalues, "ovr_hip_set_isosurface_layers", false,  true,  false, true,  true,  true,  false, 8, 8, true },
};
// the eighth entry, ovr_hip_preintegrated_floats (added with pre-integrated classification), walks the same path by a row of its own, OUTSIDE kRayQueries: that
// table stays the seven rows tests/test_ray_query_table.py holds it to.  Its id follows theirs; ray_query_row is the one lookup of a row by id
constexpr int kQueryPreintegrated = kRayQueryCount, kRayQueryIds = kRayQueryCount + 1;
constexpr RayQuery kPreintegrationQueries[1] = {
  { "ovr_hip_preintegrated_floats",      FrameKind::PreintegratedMarch, QueryNeeds::Nothing,  nullptr,                         false,  false, true,  false, false, false, false, 8, 0, false, true },
};
// the ninth, ovr_hip_gradient_opacity_floats (added with gradient opacity), likewise: a row of its own behind the pre-integration's, whose ids stay what they were
constexpr int kQueryGradientOpacity = kRayQueryIds, kRayQueryRows = kRayQueryIds + 1;
constexpr RayQuery kGradientOpacityQueries[1] = {
  { "ovr_hip_gradient_opacity_floats",   FrameKind::GradientOpacityMarch, QueryNeeds::Nothing, nullptr,                        false,  false, true,  false, false, false, false, 8, 0, false, false, true, true },
};
// the tenth, ovr_hip_max_depth_floats (added with the depth limit), likewise: a row of its own behind the gradient opacity's, whose ids stay what they were.  It
// needs nothing committed but volume and transfer function: the depths are the caller's
constexpr int kQueryMaxDepth = kRayQueryRows, kRayQueryAll = kRayQueryRows + 1;
constexpr RayQuery kMaxDepthQueries[1] = {
  { "ovr_hip_max_depth_floats",          FrameKind::DepthLimitedMarch, QueryNeeds::Nothing,   nullptr,                         false,  false, true,  false, false, false, false, 8, 0, false, false, false, true, true },
};
// the eleventh, ovr_hip_depth_output_floats (added with the depth layer), likewise: a row of its own behind the depth limit's, whose ids stay what they were.
// It needs nothing committed but volume and transfer function: depths (or none) and threshold are the caller's
constexpr int kQueryDepthOutput = kRayQueryAll, kRayQueryTotal = kRayQueryAll + 1;
constexpr RayQuery kDepthOutputQueries[1] = {
  { "ovr_hip_depth_output_floats",       FrameKind::DepthOutputMarch,  QueryNeeds::Nothing,   nullptr,                         false,  false, true,  false, false, false, false, 12, 0, false, false, false, true, true, true, true },
};
constexpr const RayQuery& ray_query_row(int id)
{
  return id >= kRayQueryAll ? kDepthOutputQueries[id - kRayQueryAll] : id >= kRayQueryRows ? kMaxDepthQueries[id - kRayQueryRows] : id >= kRayQueryIds ? kGradientOpacityQueries[id - kRayQueryIds] : id >= kRayQueryCount ? kPreintegrationQueries[id - kRayQueryCount] : kRayQueries[id];
}
// the plan a query asked for is the plan of its kernel (slices: the committed set decides between the two slice kernels, as it does for a frame)
constexpr bool query_runs(const RayQuery& d, FrameKind k) { return k == d.kind || (d.kind == FrameKind::SliceWalk && k == FrameKind::SlicePlane); }

// floats per ray of an entry's record (max_events is read where the entry takes it)
constexpr size_t ray_query_record_floats(const RayQuery& d, int max_events) { return (size_t)d.header_floats + (size_t)d.event_floats * (size_t)(d.takes_max_events ? max_events : 0); }

// a call's arguments; an entry passes 0 for what it does not take
struct RayQueryCall {
  const float* org = nullptr;
  const float* dir = nullptr;
  float* out = nullptr;
  long long n = 0;
  int mode = 0, max_events = 0, rotation = 0, range_skipping = 0;
  const float* depth = nullptr; // (takes_depth)
  float threshold = 0.f;        // (takes_threshold)
};
// what the preconditions read of the committed state
struct QueryFacts {
  bool volume = false;
  int slices = 0, isovalues = 0;
  bool slice_context = false, isosurface_context = false; // committed in mode FRONT / VOLUME
  int ao_samples = 0;
  bool transfer_function = false;   // both tables are resident
  bool ranges = false;              // the resident volume has its macrocells' value ranges
  bool preintegration = false;      // committed in mode SEGMENTS
  bool gradient_opacity = false;    // committed in mode RAMP
};
struct QueryStatus { int code = 0; std::string message; };
inline QueryStatus query_refusal(const RayQuery& d, int code, const std::string& what) { return { code, std::string("[hip] ") + d.name + ": " + what }; }

// step one of an entry, in front of anything that touches the device
inline QueryStatus ray_query_arguments(const RayQuery& d, bool renderer, const RayQueryCall& c)
{
  const bool bad = !renderer || !c.org || !c.dir || !c.out || c.n < 0 || (d.takes_mode && (c.mode < kProjectMaximum || c.mode > kProjectMean)) || (d.takes_shade && (c.mode < 0 || c.mode > 1)) || (d.takes_depth && !d.depth_optional && !c.depth)
                   || (d.takes_threshold && depth_output_check(kDepthOutputOn, c.threshold) != kDepthOutputOk)
                   || (d.takes_max_events && (c.max_events < 1 || c.max_events > kQueryMaxEvents)) || (d.takes_rotation && (c.rotation < 0 || c.rotation >= kQueryRotations));
  return bad ? query_refusal(d, kQueryEinval, "bad arguments") : QueryStatus();
}

// the preconditions, reported in this order: volume, slices or isovalues, context mode, AO samples, pre-integration, gradient opacity, transfer function, macrocell ranges
inline QueryStatus ray_query_preconditions(const RayQuery& d, const QueryFacts& f, bool range_skipping)
{
  const bool slices = d.needs == QueryNeeds::Slices;
  if (!f.volume) return query_refusal(d, kQueryEstate, "no volume was set");
  if (slices && f.slices < 1) return query_refusal(d, kQueryEstate, std::string("no slice is committed (") + d.setter + ")");
  if (d.needs == QueryNeeds::Isovalues && f.isovalues < 1) return query_refusal(d, kQueryEstate, std::string("no isovalue is committed (") + d.setter + ")");
  if (d.needs_context && !(slices ? f.slice_context : f.isosurface_context))
    return query_refusal(d, kQueryEstate, slices ? "no slice context is committed (ovr_hip_set_slice_context)" : "no isosurface context is committed (ovr_hip_set_isosurface_context)");
  if (d.needs_ao && f.ao_samples < 1) return query_refusal(d, kQueryEstate, "no ambient-occlusion sample is committed (ovr_hip_set_ambient_occlusion)");
  if (d.needs_preintegration && !f.preintegration) return query_refusal(d, kQueryEstate, "no pre-integration is committed (ovr_hip_set_preintegration)");
  if (d.needs_gradient_opacity && !f.gradient_opacity) return query_refusal(d, kQueryEstate, "no gradient opacity is committed (ovr_hip_set_gradient_opacity)");
  if (d.needs_tf && !f.transfer_function) return query_refusal(d, kQueryEstate, "no transfer function was committed");
  if (d.takes_range_skipping && range_skipping && !f.ranges) return query_refusal(d, kQueryEstate, "the resident volume has no macrocell ranges");
  return QueryStatus();
}

} // namespace ovrhip
