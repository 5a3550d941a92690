// ovr_hip_depth_output.hip - the depth-output kernels of one voxel type of the general layout (explicit instantiation; see ovr_hip_depth_output.h).
// Compiled once per such type with -DOVR_MARCH_VT=<its enumerator>, each into an object of its own beside the type's march, isosurface, slice, context,
// pre-integration, gradient-opacity and depth-limit objects (Makefile), which are what they were
#include "ovr_hip_depth_output.h"

#ifndef OVR_MARCH_VT
#error "compile this unit once per general-layout entry of OVR_VOXEL_TYPES, with the entry's VoxelType enumerator as the value of the OVR_MARCH_VT define (see the Makefile)"
#endif

namespace ovrhip {
static_assert(kVoxelTypes[OVR_MARCH_VT].layout == LAYOUT_GENERAL, "the depth-output kernels read the general layout");
template DepthOutputKernels depth_output_kernels_of<OVR_MARCH_VT>(const LaunchPlan&);
}
