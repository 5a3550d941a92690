// ovr_hip_march.hip - the march / shade kernels of one voxel type (explicit instantiation; see ovr_hip_device.h).  Compiled once per
// entry of OVR_VOXEL_TYPES (ovr_hip_kernels.h) with -DOVR_MARCH_VT=<its enumerator>, each into an object of its own (Makefile)
#include "ovr_hip_device.h"

#ifndef OVR_MARCH_VT
#error "compile this unit once per entry of OVR_VOXEL_TYPES, with the entry's VoxelType enumerator as the value of the OVR_MARCH_VT define (see the Makefile)"
#endif

namespace ovrhip {
template FrameKernels frame_kernels<OVR_MARCH_VT>(const LaunchPlan&);
template ShadowCacheKernel shadow_cache_kernel_of<OVR_MARCH_VT>(int);
template ProjectKernels project_kernels_of<OVR_MARCH_VT>(const LaunchPlan&);
}
