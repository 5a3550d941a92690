// plan_compare.hpp - what "the same plan" means in every plan driver of this directory: one comparison of every member of a LaunchPlan
// (csrc/host/launch_plan.hpp).  A driver's "the same but for X" copies both plans, equalises the X members and asks same_plan - so a member added to the plan
// is compared by every driver from the day it is added here.
#pragma once

#include "launch_plan.hpp"

namespace ovrhip {

inline bool same_plan(const LaunchPlan& a, const LaunchPlan& b)
{
  return a.shading == b.shading && a.am == b.am && a.pooled == b.pooled && a.skip == b.skip
         && a.march.lds_staged == b.march.lds_staged && a.march.deep == b.march.deep && a.march.material == b.march.material && a.march.clipped == b.march.clipped
         && a.shade.material == b.shade.material && a.shade.clipped == b.shade.clipped
         && a.shade_order == b.shade_order && a.orthographic == b.orthographic && a.cached == b.cached
         && a.project.mode == b.project.mode && a.project.skip == b.project.skip && a.project.clipped == b.project.clipped && a.project.lds_bytes == b.project.lds_bytes
         && a.isosurface.on == b.isosurface.on && a.isosurface.skip == b.isosurface.skip && a.isosurface.clipped == b.isosurface.clipped
         && a.isosurface.lds_bytes == b.isosurface.lds_bytes && a.isosurface.translucent == b.isosurface.translucent && a.isosurface.context == b.isosurface.context
         && a.march_lds_bytes == b.march_lds_bytes && a.shade_lds_bytes == b.shade_lds_bytes && a.lds_brick_offset == b.lds_brick_offset
         && a.shade_grid_blocks == b.shade_grid_blocks && a.error == b.error && a.ambient_occlusion == b.ambient_occlusion
         && a.slices.on == b.slices.on && a.slices.walks == b.slices.walks && a.slices.skip == b.slices.skip && a.slices.clipped == b.slices.clipped
         && a.slices.lds_bytes == b.slices.lds_bytes && a.slices.context == b.slices.context;
}

} // namespace ovrhip
