// update_extent.hpp - the host arithmetic of ovr_hip_update_volume: which part of each resident layout, and which macrocells,
// hold a copy of a voxel of the box [lower, lower + extent) - and the argument checks.  Like policy.hpp nothing here calls HIP or knows the renderer:
// volume.cpp sizes the launches with it, the kernels apply the per-row predicates, and tests/volume_update_driver.cpp compares every range with a
// brute-force enumeration of "this stored element is a copy of a voxel in the box" on a machine without a GPU.
#pragma once

#include <algorithm>
#include <cstdint>

namespace ovrhip {
namespace update {

struct Box { int lo[3], hi[3]; }; // voxels [lo, hi) per axis (x, y, z)

// a layout's brick geometry: Vox<>'s cx / mbx / by / bz as numbers (ovr_hip_device.h); transposed = the pair axis is the volume's y
struct Geometry { int cx, mbx, by, bz; bool transposed, quad; int lx, ly, lz; };

enum { kOk = 0, kNull = 1, kMemKind = 2, kType = 3, kExtent = 4, kOutside = 5 };
// the argument checks of ovr_hip_update_volume (everything but "is a volume set"): 0, or which of the EINVAL rules is broken
inline int check_arguments(const void* data, const int32_t* lower, const int32_t* extent, int mem_kind, int value_type, int resident_type, const int dims[3])
{
  if (!data || !lower || !extent) return kNull;
  if (mem_kind != 0 && mem_kind != 1) return kMemKind; // OVR_HIP_MEM_HOST / OVR_HIP_MEM_DEVICE
  if (value_type != resident_type) return kType;
  for (int k = 0; k < 3; ++k)
    if (extent[k] < 1) return kExtent;
  for (int k = 0; k < 3; ++k)
    if (lower[k] < 0 || lower[k] >= dims[k] || extent[k] > dims[k] - lower[k]) return kOutside;
  return kOk;
}
inline const char* check_text(int rule)
{
  switch (rule) {
  case kNull: return "null argument";
  case kMemKind: return "bad mem_kind";
  case kType: return "value_type is not the resident volume's";
  case kExtent: return "extent must be positive";
  case kOutside: return "the box leaves the grid";
  default: return "";
  }
}

// ---- bricked layouts (general, thin): a stored element (brick br along the pair axis, k = 0 ... cx) is a copy of voxel clamp(br * cx - 1 + k, 0, na - 1)
struct BrickRange {
  int brick_lo, brick_hi;   // bricks along the pair axis whose stored span meets the box (inclusive)
  int macro_lo, macro_hi;   // ... the macro blocks they lie in
  int row_lo, row_hi;       // macro rows (32 voxels) along the other in-plane axis
  int layer_lo, layer_hi;   // z layers (2^bz slices)
};

// bricks_total = macros_a * mbx: the bricks the layout stores along the pair axis
inline void pair_axis_bricks(int cx, int na, int bricks_total, int a, int b, int& lo, int& hi)
{
  // stored position p holds voxel clamp(p - 1): the box's voxels [a, b) are positions a + 1 ... b, plus position 0 with voxel 0 and every position
  // past the grid with voxel na - 1; brick br stores positions br * cx ... br * cx + cx (the last one duplicates the next brick's first)
  const int p_lo = a == 0 ? 0 : a + 1;
  lo = p_lo == 0 ? 0 : (p_lo - 1) / cx;
  hi = b == na ? bricks_total - 1 : std::min(b / cx, bricks_total - 1);
}

inline BrickRange brick_range(const Geometry& g, const int dims[3], int macros_a, const Box& box)
{
  const int ia = g.transposed ? 1 : 0, ib = g.transposed ? 0 : 1;
  BrickRange r;
  pair_axis_bricks(g.cx, dims[ia], macros_a * g.mbx, box.lo[ia], box.hi[ia], r.brick_lo, r.brick_hi);
  r.macro_lo = r.brick_lo / g.mbx; r.macro_hi = r.brick_hi / g.mbx;
  r.row_lo = box.lo[ib] >> 5; r.row_hi = (box.hi[ib] - 1) >> 5;
  r.layer_lo = box.lo[2] >> g.bz; r.layer_hi = (box.hi[2] - 1) >> g.bz;
  return r;
}

// ---- quad replicas: cell (u, v) holds the voxels x in { max(u - 1, 0), min(u, nx - 1) }, y likewise: the box grown by one cell
struct QuadRange {
  int u_lo, u_hi, v_lo, v_hi; // cells (inclusive)
  int macro_lo, macro_hi;     // macro blocks along x (32 cells)
  int row_lo, row_hi;         // macro rows along y
  int layer_lo, layer_hi;     // z layers (2^lz slices)
};
inline QuadRange quad_range(const Geometry& g, const Box& box)
{
  QuadRange r;
  r.u_lo = box.lo[0]; r.u_hi = box.hi[0];
  r.v_lo = box.lo[1]; r.v_hi = box.hi[1];
  r.macro_lo = r.u_lo >> 5; r.macro_hi = r.u_hi >> 5;
  r.row_lo = r.v_lo >> 5; r.row_hi = r.v_hi >> 5;
  r.layer_lo = box.lo[2] >> g.lz; r.layer_hi = (box.hi[2] - 1) >> g.lz;
  return r;
}

// ---- macrocells: cell c reads the voxels [max(16 c - 1, 0), max(16 c - 1, 0) + 17) of its axis (macrocell_range_kernel; the reference clamps the
// lower end before it adds the width, so cell 0's window is voxels 0 ... 16 and voxel 16 belongs to cells 0 AND 1)
inline void macrocell_axis(int n, int a, int b, int& lo, int& hi)
{
  const int cells = (n + 15) / 16;
  lo = a <= 16 ? 0 : a >> 4;
  hi = std::min(b >> 4, cells - 1);
}
struct CellRange { int lo[3], hi[3]; }; // inclusive
inline CellRange macrocell_range(const int dims[3], const Box& box)
{
  CellRange c;
  for (int k = 0; k < 3; ++k) macrocell_axis(dims[k], box.lo[k], box.hi[k], c.lo[k], c.hi[k]);
  return c;
}

} // namespace update
} // namespace ovrhip
