// ovr_hip_isosurface.hip - the isosurface kernels of one voxel type of the general layout (explicit instantiation; see ovr_hip_device.h).  Compiled once per such
// type with -DOVR_MARCH_VT=<its enumerator>, each into an object of its own beside the type's march object (Makefile): the march objects are what they were
// With -DOVR_ISO_LAYERS the unit instantiates the type's TRANSLUCENT kernels instead, into a second object per type: the opaque kernels'
// object is compiled from what it was compiled from, and the two compile in parallel
// With -DOVR_ISO_AO the unit instantiates the type's AMBIENT-OCCLUSION kernels instead (ovr_hip_isosurface_ao.h), into a third object per type
#ifdef OVR_ISO_AO
#include "ovr_hip_isosurface_ao.h"
#else
#include "ovr_hip_device.h"
#endif

#ifndef OVR_MARCH_VT
#error "compile this unit once per general-layout entry of OVR_VOXEL_TYPES, with the entry's VoxelType enumerator as the value of the OVR_MARCH_VT define (see the Makefile)"
#endif

namespace ovrhip {
static_assert(kVoxelTypes[OVR_MARCH_VT].layout == LAYOUT_GENERAL, "the isosurface kernels read the general layout");
#if defined(OVR_ISO_AO)
template IsosurfaceAoKernels isosurface_ao_kernels_of<OVR_MARCH_VT>(const LaunchPlan&);
#elif defined(OVR_ISO_LAYERS)
template IsosurfaceLayersKernels isosurface_kernels_of<OVR_MARCH_VT, true>(const LaunchPlan&);
#else
template IsosurfaceKernels isosurface_kernels_of<OVR_MARCH_VT, false>(const LaunchPlan&);
#endif
}
