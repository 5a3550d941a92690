// volume_update_driver.cpp - csrc/host/update_extent.hpp against brute force (tests/test_volume_update_model.py builds this with the host compiler
// against that header alone).  For a layout geometry given as numbers (Vox<>'s cx / mbx / by / bz, or a quad replica's lx / ly / lz) every stored
// element of the layout is enumerated on four grids and asked "are you a copy of a voxel in the box": every copy must lie inside the header's
// ranges, and every end of every range must be reached by a copy.
//   driver brick <cx> <mbx> <by> <bz> <transposed>     driver quad <lx> <ly> <lz>     driver cells     driver args     driver boxes
#include "update_extent.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ovrhip::update;

static const int kGrids[4][3] = { { 1, 1, 1 }, { 3, 2, 5 }, { 31, 33, 17 }, { 70, 67, 69 } };
static int g_failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (g_failures++ < 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static unsigned g_seed = 20261018u;
static int rnd(int n) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (unsigned)n); }

// the seeded box set of a grid: single voxels at the eight corners, boxes touching each face, the whole grid, boxes ending at 16 k - 1, 16 k and
// 16 k + 1 on every axis (and starting there), and random ones
static std::vector<Box> boxes_of(const int n[3])
{
  std::vector<Box> out;
  auto add = [&](int x0, int x1, int y0, int y1, int z0, int z1) {
    Box b{ { x0, y0, z0 }, { x1, y1, z1 } };
    for (int k = 0; k < 3; ++k) {
      b.lo[k] = std::min(std::max(b.lo[k], 0), n[k] - 1);
      b.hi[k] = std::min(std::max(b.hi[k], b.lo[k] + 1), n[k]);
    }
    out.push_back(b);
  };
  for (int c = 0; c < 8; ++c) {
    const int x = (c & 1) ? n[0] - 1 : 0, y = (c & 2) ? n[1] - 1 : 0, z = (c & 4) ? n[2] - 1 : 0;
    add(x, x + 1, y, y + 1, z, z + 1);
  }
  const int m[3] = { n[0] / 2, n[1] / 2, n[2] / 2 };
  for (int k = 0; k < 3; ++k)
    for (int side = 0; side < 2; ++side) { // a slab of up to 3 voxels on the face, a third of the grid wide across
      int lo[3] = { m[0] - n[0] / 6, m[1] - n[1] / 6, m[2] - n[2] / 6 }, hi[3] = { m[0] + n[0] / 6 + 1, m[1] + n[1] / 6 + 1, m[2] + n[2] / 6 + 1 };
      lo[k] = side ? n[k] - 3 : 0; hi[k] = side ? n[k] : 3;
      add(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]);
    }
  add(0, n[0], 0, n[1], 0, n[2]);
  for (int k = 0; k < 3; ++k)
    for (int e = 15; e <= n[k] + 1; e += 16)
      for (int d = 0; d < 3; ++d) {
        int lo[3] = { rnd(n[0]), rnd(n[1]), rnd(n[2]) }, hi[3];
        for (int j = 0; j < 3; ++j) hi[j] = lo[j] + 1 + rnd(n[j]);
        lo[k] = std::max(e + d - 1 - rnd(20), 0); hi[k] = e + d; // ends at 16 k - 1, 16 k, 16 k + 1
        add(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]);
        lo[k] = e + d; hi[k] = e + d + 1 + rnd(20);              // ... and starts there
        add(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]);
      }
  for (int i = 0; i < 40; ++i) {
    int lo[3] = { rnd(n[0]), rnd(n[1]), rnd(n[2]) };
    add(lo[0], lo[0] + 1 + rnd(n[0]), lo[1], lo[1] + 1 + rnd(n[1]), lo[2], lo[2] + 1 + rnd(n[2]));
  }
  return out;
}

struct MinMax {
  int lo = INT_MAX, hi = INT_MIN;
  void add(int v) { lo = std::min(lo, v); hi = std::max(hi, v); }
};
static bool inside(int v, int lo, int hi) { return v >= lo && v < hi; }
static int clampi(int v, int lo, int hi) { return std::min(std::max(v, lo), hi); }

static int run_brick(int cx, int mbx, int by, int bz, bool tr)
{
  const Geometry g{ cx, mbx, by, bz, tr, false, 0, 0, 0 };
  int n_boxes = 0;
  for (const auto& n : kGrids) {
    const int ia = tr ? 1 : 0, ib = tr ? 0 : 1;
    const int na = n[ia], nb = n[ib], nz = n[2];
    const int macros_a = (na + 1 + cx * mbx - 1) / (cx * mbx); // volume_layout_t
    const int macros_b = (nb + 31) / 32, macros_z = (nz + 31) / 32;
    for (const Box& box : boxes_of(n)) {
      ++n_boxes;
      const BrickRange r = brick_range(g, n, macros_a, box);
      MinMax brick, macro, row, layer;
      long copies = 0;
      for (int z = 0; z < macros_z * 32; ++z)
        for (int b = 0; b < macros_b * 32; ++b)
          for (int br = 0; br < macros_a * mbx; ++br)
            for (int k = 0; k <= cx; ++k) {
              // rows beyond the grid (b >= nb, z >= nz) are padding: copies of nothing
              const bool copy = b < nb && z < nz && inside(clampi(br * cx - 1 + k, 0, na - 1), box.lo[ia], box.hi[ia]) && inside(b, box.lo[ib], box.hi[ib]) &&
                                inside(z, box.lo[2], box.hi[2]);
              if (!copy) continue;
              ++copies;
              brick.add(br); macro.add(br / mbx); row.add(b >> 5); layer.add(z >> bz);
              EXPECT(br >= r.brick_lo && br <= r.brick_hi && br / mbx >= r.macro_lo && br / mbx <= r.macro_hi && (b >> 5) >= r.row_lo && (b >> 5) <= r.row_hi &&
                         (z >> bz) >= r.layer_lo && (z >> bz) <= r.layer_hi,
                     "grid %dx%dx%d box [%d,%d)x[%d,%d)x[%d,%d): element brick %d k %d b %d z %d is outside the ranges", n[0], n[1], n[2], box.lo[0], box.hi[0],
                     box.lo[1], box.hi[1], box.lo[2], box.hi[2], br, k, b, z);
            }
      EXPECT(copies > 0, "no copies");
      EXPECT(brick.lo == r.brick_lo && brick.hi == r.brick_hi, "grid %dx%dx%d box a [%d,%d): bricks %d..%d, header %d..%d", n[0], n[1], n[2], box.lo[ia], box.hi[ia], brick.lo,
             brick.hi, r.brick_lo, r.brick_hi);
      EXPECT(macro.lo == r.macro_lo && macro.hi == r.macro_hi, "macro blocks %d..%d, header %d..%d", macro.lo, macro.hi, r.macro_lo, r.macro_hi);
      EXPECT(row.lo == r.row_lo && row.hi == r.row_hi, "macro rows %d..%d, header %d..%d", row.lo, row.hi, r.row_lo, r.row_hi);
      EXPECT(layer.lo == r.layer_lo && layer.hi == r.layer_hi, "layers %d..%d, header %d..%d", layer.lo, layer.hi, r.layer_lo, r.layer_hi);
      EXPECT(r.macro_hi < macros_a && r.row_hi < macros_b && r.layer_hi < macros_z * (32 >> bz), "a range leaves the layout");
    }
  }
  std::printf("brick cx=%d mbx=%d by=%d bz=%d tr=%d: %d boxes\n", cx, mbx, by, bz, (int)tr, n_boxes);
  return n_boxes;
}

static int run_quad(int lx, int ly, int lz)
{
  const Geometry g{ 1 << lx, 32 >> lx, ly, lz, false, true, lx, ly, lz };
  int n_boxes = 0;
  for (const auto& n : kGrids) {
    const int macros_x = (n[0] + 1 + 31) / 32, macros_y = (n[1] + 1 + 31) / 32, macros_z = (n[2] + 31) / 32; // volume_layout_t: cells 0 ... n on x and y
    for (const Box& box : boxes_of(n)) {
      ++n_boxes;
      const QuadRange r = quad_range(g, box);
      MinMax cu, cv, macro, row, layer;
      for (int z = 0; z < macros_z * 32; ++z)
        for (int v = 0; v < macros_y * 32; ++v)
          for (int u = 0; u < macros_x * 32; ++u) {
            if (u > n[0] || v > n[1] || z >= n[2]) continue; // a padding cell
            const int x0 = std::max(u - 1, 0), x1 = std::min(u, n[0] - 1), y0 = std::max(v - 1, 0), y1 = std::min(v, n[1] - 1);
            const bool copy = (inside(x0, box.lo[0], box.hi[0]) || inside(x1, box.lo[0], box.hi[0])) && (inside(y0, box.lo[1], box.hi[1]) || inside(y1, box.lo[1], box.hi[1])) &&
                              inside(z, box.lo[2], box.hi[2]);
            if (!copy) continue;
            cu.add(u); cv.add(v); macro.add(u >> 5); row.add(v >> 5); layer.add(z >> lz);
          }
      EXPECT(cu.lo == r.u_lo && cu.hi == r.u_hi && cv.lo == r.v_lo && cv.hi == r.v_hi, "grid %dx%dx%d box [%d,%d)x[%d,%d): cells %d..%d x %d..%d, header %d..%d x %d..%d", n[0],
             n[1], n[2], box.lo[0], box.hi[0], box.lo[1], box.hi[1], cu.lo, cu.hi, cv.lo, cv.hi, r.u_lo, r.u_hi, r.v_lo, r.v_hi);
      EXPECT(macro.lo == r.macro_lo && macro.hi == r.macro_hi && row.lo == r.row_lo && row.hi == r.row_hi, "macro blocks / rows");
      EXPECT(layer.lo == r.layer_lo && layer.hi == r.layer_hi, "layers %d..%d, header %d..%d", layer.lo, layer.hi, r.layer_lo, r.layer_hi);
      EXPECT(r.macro_hi < macros_x && r.row_hi < macros_y && r.layer_hi < macros_z * (32 >> lz), "a range leaves the layout");
    }
  }
  std::printf("quad lx=%d ly=%d lz=%d: %d boxes\n", lx, ly, lz, n_boxes);
  return n_boxes;
}

static int run_cells()
{
  int n_boxes = 0;
  for (const auto& n : kGrids)
    for (const Box& box : boxes_of(n)) {
      ++n_boxes;
      const CellRange r = macrocell_range(n, box);
      for (int k = 0; k < 3; ++k) {
        MinMax c;
        for (int cell = 0; cell < (n[k] + 15) / 16; ++cell) { // macrocell_range_kernel: bx = max(16 c - 1, 0), ex = min(bx + 17, n)
          const int b0 = std::max(16 * cell - 1, 0), e0 = std::min(b0 + 17, n[k]);
          if (b0 < box.hi[k] && box.lo[k] < e0) c.add(cell);
        }
        EXPECT(c.lo == r.lo[k] && c.hi == r.hi[k], "axis %d of %d, box [%d,%d): cells %d..%d, header %d..%d", k, n[k], box.lo[k], box.hi[k], c.lo, c.hi, r.lo[k], r.hi[k]);
      }
    }
  std::printf("cells: %d boxes\n", n_boxes);
  return n_boxes;
}

static int run_args()
{
  const int dims[3] = { 70, 67, 69 };
  const int32_t lo[3] = { 1, 2, 3 }, ext[3] = { 4, 5, 6 };
  int x = 0;
  EXPECT(check_arguments(&x, lo, ext, 0, 400, 400, dims) == kOk, "a good call");
  EXPECT(check_arguments(&x, lo, ext, 1, 400, 400, dims) == kOk, "a good call from device memory");
  EXPECT(check_arguments(nullptr, lo, ext, 0, 400, 400, dims) == kNull && check_arguments(&x, nullptr, ext, 0, 400, 400, dims) == kNull &&
             check_arguments(&x, lo, nullptr, 0, 400, 400, dims) == kNull, "null");
  EXPECT(check_arguments(&x, lo, ext, 2, 400, 400, dims) == kMemKind && check_arguments(&x, lo, ext, -1, 400, 400, dims) == kMemKind, "mem_kind");
  EXPECT(check_arguments(&x, lo, ext, 0, 500, 400, dims) == kType, "type");
  for (int k = 0; k < 3; ++k) {
    int32_t e[3] = { 4, 5, 6 }, l[3] = { 1, 2, 3 };
    e[k] = 0;
    EXPECT(check_arguments(&x, l, e, 0, 400, 400, dims) == kExtent, "extent 0");
    e[k] = -3;
    EXPECT(check_arguments(&x, l, e, 0, 400, 400, dims) == kExtent, "extent < 0");
    e[k] = dims[k] - l[k];
    EXPECT(check_arguments(&x, l, e, 0, 400, 400, dims) == kOk, "a box that ends at the grid's face");
    e[k] = dims[k] - l[k] + 1;
    EXPECT(check_arguments(&x, l, e, 0, 400, 400, dims) == kOutside, "one voxel past the face");
    e[k] = INT32_MAX;
    EXPECT(check_arguments(&x, l, e, 0, 400, 400, dims) == kOutside, "an extent whose sum with lower overflows");
    e[k] = 1; l[k] = -1;
    EXPECT(check_arguments(&x, l, e, 0, 400, 400, dims) == kOutside, "lower < 0");
    l[k] = dims[k];
    EXPECT(check_arguments(&x, l, e, 0, 400, 400, dims) == kOutside, "lower == n");
    l[k] = dims[k] - 1;
    EXPECT(check_arguments(&x, l, e, 0, 400, 400, dims) == kOk, "the last voxel");
  }
  std::printf("args\n");
  return 1;
}

// the box set must hold what the test promises
static int run_boxes()
{
  const int* n = kGrids[3];
  bool whole = false, corners[8] = {}, faces[6] = {}, ends[3][3] = {};
  for (const Box& b : boxes_of(n)) {
    bool w = true;
    for (int k = 0; k < 3; ++k) w = w && b.lo[k] == 0 && b.hi[k] == n[k];
    whole = whole || w;
    if (b.hi[0] - b.lo[0] == 1 && b.hi[1] - b.lo[1] == 1 && b.hi[2] - b.lo[2] == 1)
      for (int c = 0; c < 8; ++c)
        if (b.lo[0] == ((c & 1) ? n[0] - 1 : 0) && b.lo[1] == ((c & 2) ? n[1] - 1 : 0) && b.lo[2] == ((c & 4) ? n[2] - 1 : 0)) corners[c] = true;
    for (int k = 0; k < 3; ++k) {
      if (b.lo[k] == 0 && !w) faces[2 * k] = true;
      if (b.hi[k] == n[k] && !w) faces[2 * k + 1] = true;
      for (int d = 0; d < 3; ++d)
        if (b.hi[k] % 16 == (15 + d) % 16) ends[k][d] = true;
    }
  }
  EXPECT(whole, "the whole grid");
  for (int c = 0; c < 8; ++c) EXPECT(corners[c], "corner %d", c);
  for (int f = 0; f < 6; ++f) EXPECT(faces[f], "face %d", f);
  for (int k = 0; k < 3; ++k)
    for (int d = 0; d < 3; ++d) EXPECT(ends[k][d], "axis %d: a box ending at 16 k %+d", k, d - 1);
  std::printf("boxes\n");
  return 1;
}

int main(int argc, char** argv)
{
  int ran = 0;
  if (argc == 7 && !std::strcmp(argv[1], "brick")) ran = run_brick(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]) != 0);
  else if (argc == 5 && !std::strcmp(argv[1], "quad")) ran = run_quad(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
  else if (argc == 2 && !std::strcmp(argv[1], "cells")) ran = run_cells();
  else if (argc == 2 && !std::strcmp(argv[1], "args")) ran = run_args();
  else if (argc == 2 && !std::strcmp(argv[1], "boxes")) ran = run_boxes();
  if (!ran) { std::printf("usage: driver brick <cx> <mbx> <by> <bz> <transposed> | quad <lx> <ly> <lz> | cells | args | boxes\n"); return 2; }
  if (g_failures) std::printf("%d failures\n", g_failures);
  return g_failures ? 1 : 0;
}
