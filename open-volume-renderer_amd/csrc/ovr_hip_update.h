// ovr_hip_update.h - launch interface of ovr_hip_update_volume's kernels: the box-restricted siblings of launch_relayout,
// launch_rebrick and launch_macrocell_ranges (ovr_hip_kernels.h; the kernels stand next to the ones they mirror in ovr_hip_kernels.hip and share
// their addressing with them: RowSweep / QuadSweep, src_bricked, dispatch_value_type).
// Internal to libovr_hip.so.
#pragma once

#include "ovr_hip_kernels.h"
#pragma GCC visibility push(hidden)
#include "host/update_extent.hpp"
#pragma GCC visibility pop

namespace ovrhip {

// src_box holds the box's voxels alone (x fastest, any reference ValueType): every stored element of the GENERAL layout dst that is a copy of a voxel
// in the box is rewritten - apron duplicates, the copy of voxel 0 and the replicas of the last voxel included -, nothing else is touched
hipError_t launch_update_general(const void* src_box, int ovr_value_type, void* dst, const VolumeDesc& vd, const update::Box& box, hipStream_t stream);
// ... and the rows / cells of a replica (vd, dst) that hold such a copy, from the general layout - which is current by then
hipError_t launch_update_replica(const VolumeDesc& general, void* dst, const VolumeDesc& vd, const update::Box& box, hipStream_t stream);
// the value ranges of the macrocells [cells.lo, cells.hi] alone: macrocell_range_kernel's arithmetic per cell, the other cells keep their range
hipError_t launch_macrocell_ranges_box(const VolumeDesc& vd, float* out_minmax, const update::CellRange& cells, hipStream_t stream);

} // namespace ovrhip
