// Driver of tests/test_launch_plan.py: runs csrc/host/launch_plan.hpp - which march / shade kernel variant a frame takes, with which LDS sizes - on the
// CPU.  `driver <scenario>` exits 0 when every row of the scenario's table gave what the row expects.  The expectations are literals: the rules as the
// launcher stated them before they were gathered in plan_launch (the nesting of its `if constexpr`s, its deep-rounds rule, its addressing rule), worked
// out by hand per row - none is computed by calling the header.  Every variant renders the same frame, so no frame test can see a wrong choice; this can.
#include "launch_plan.hpp"

#include <cstdio>
#include <cstring>

using namespace ovrhip;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("]\n"); } \
  } while (0)

typedef unsigned long long u64;
constexpr u64 GiB4 = 0x100000000ull;

// a 24^3 volume of the general f32 layout under a 256 / 256 transfer function: small, 32-bit byte offsets (mode 0)
static LaunchFacts f32_24()
{
  LaunchFacts f;
  f.elem_bytes = 4; f.f32_general = true;
  f.nx = f.ny = f.nz = 24;
  f.stored_bytes = 1u << 20;
  f.n_color = f.n_alpha = 256;
  f.n_blocks_owned = f.n_schedule = 96;
  return f;
}
static LaunchOverrides ov(int addressing, int deep = -1, int shade_blocks = 0) { LaunchOverrides o; o.addressing = addressing; o.deep = deep; o.shade_blocks = shade_blocks; return o; }

static void addressing()
{
  // stored bytes, element size, dims, TF entries (colour = alpha) -> mode
  struct Row { const char* what; u64 bytes; int elem, nx, ny, nz, tf, am; };
  const Row rows[] = {
    { "4 GiB exactly: byte offsets", GiB4, 4, 2048, 2048, 256, 256, 0 },
    { "one element past 4 GiB: element offsets", GiB4 + 4, 4, 2048, 2048, 257, 256, 1 },
    { "2^32 - 2 stored elements", 4 * 0xfffffffeull, 4, 2048, 2048, 1024, 256, 1 },
    { "2^32 - 1 stored elements: 64-bit z table", 4 * 0xffffffffull, 4, 2048, 2048, 1024, 256, 2 },
    { "8-bit voxels, 2^32 - 1 bytes", 0xffffffffull, 1, 2048, 2048, 1024, 256, 0 },
    { "8-bit voxels, 2^32 + 1 bytes: 2^32 + 1 elements", GiB4 + 1, 1, 2048, 2048, 1024, 256, 2 },
    // mode 2's tables: 8 (nz + 2) + 4 (nx + ny + 3).  nz 7000: 56016 + 8012 = 64028 <= 65536; nz 8000: 64016 + 8012 = 72028 > 65536, while
    // 72028 + 16 + (TF 5152 + queues 32768 + 1024) = 110988 <= 163840: the first condition alone
    { "mode 2, tables of 64028 bytes", 4 * 0xffffffffull, 4, 1000, 1000, 7000, 256, 2 },
    { "mode 2, tables of 72028 bytes: computed", 4 * 0xffffffffull, 4, 1000, 1000, 8000, 256, 3 },
    // the case tests/test_round3_gpu.py pins: 24000 x 6 x 5 voxels of 8 bits.  Tables 4 (24009 + 7) = 96064; TF 4096 x 16 + 4096 x 4 + 32 = 81952;
    // 96064 + 16 + 81952 + 32768 + 1024 = 211824 > 163840.  Under 256 entries: 96064 + 16 + 5152 + 32768 + 1024 = 135024 <= 163840
    { "a 24000-voxel axis under 4096 TF entries: computed", 1u << 20, 1, 24000, 6, 5, 4096, 3 },
    { "a 24000-voxel axis under 256 TF entries", 1u << 20, 1, 24000, 6, 5, 256, 0 },
  };
  for (const Row& r : rows) {
    CHECK(addressing_mode(r.bytes, r.elem, r.nx, r.ny, r.nz, r.tf, r.tf) == r.am, "%s: mode %d, expected %d", r.what, addressing_mode(r.bytes, r.elem, r.nx, r.ny, r.nz, r.tf, r.tf), r.am);
    LaunchFacts f = f32_24();
    f.elem_bytes = r.elem; f.f32_general = r.elem == 4; f.stored_bytes = r.bytes; f.nx = r.nx; f.ny = r.ny; f.nz = r.nz; f.n_color = f.n_alpha = r.tf;
    f.row_loads = 1; // (8-bit voxels past 128 MiB would take the row loads: the next scenario)
    const LaunchPlan p = plan_launch(f);
    CHECK(!p.error && p.am == r.am, "%s: the plan's mode %d (error %d), expected %d", r.what, p.am, (int)p.error, r.am);
  }
  // the override: max(mode, k), at most 3
  struct Ov { u64 bytes; int k, am; };
  const Ov ovs[] = { { 1u << 20, 0, 0 }, { 1u << 20, 1, 1 }, { 1u << 20, 2, 2 }, { 1u << 20, 3, 3 }, { 1u << 20, 7, 3 }, { GiB4 + 4, 0, 1 }, { GiB4 + 4, 2, 2 },
                     { 4 * 0xffffffffull, 1, 2 }, { 4 * 0xffffffffull, 3, 3 } };
  for (const Ov& r : ovs) {
    LaunchFacts f = f32_24();
    f.stored_bytes = r.bytes;
    const LaunchPlan p = plan_launch(f, ov(r.k));
    CHECK(!p.error && p.am == r.am, "override %d on %llu bytes: mode %d, expected %d", r.k, r.bytes, p.am, r.am);
  }
  // modes 0 ... 2 read the layout's tables; mode 3 does not
  for (int k = 0; k <= 3; ++k) {
    LaunchFacts f = f32_24();
    f.tables = false;
    CHECK(plan_launch(f, ov(k)).error == (k < 3), "no tables at mode %d: error %d", k, (int)plan_launch(f, ov(k)).error);
  }
}

static void row_loads()
{
  constexpr u64 MiB128 = 128ull << 20;
  // element size, quad, stored bytes, row_loads (0 by size, 1 never, 2 always), addressing override -> mode
  struct Row { int elem; bool quad; u64 bytes; int row_loads, k, am; };
  const Row rows[] = {
    { 2, false, MiB128, 0, -1, 0 },     { 2, false, MiB128 + 2, 0, -1, 4 }, { 1, false, MiB128 + 1, 0, -1, 4 }, { 1, false, MiB128, 0, -1, 0 },
    { 2, false, MiB128 + 2, 1, -1, 0 }, { 2, false, 1u << 20, 1, -1, 0 },   { 2, false, 1u << 20, 2, -1, 4 },   { 1, false, 1u << 20, 2, -1, 4 },
    { 4, false, MiB128 + 4, 0, -1, 0 }, { 4, false, 1u << 20, 2, -1, 0 },   // 32-bit voxels: never
    { 2, true, MiB128 + 2, 0, -1, 0 },  { 2, true, 1u << 20, 2, -1, 0 },    { 1, true, 1u << 20, 2, -1, 0 },    // quad layouts: never
    { 2, false, GiB4 + 2, 0, -1, 1 },   { 2, false, GiB4 + 2, 2, -1, 1 },   // mode 0 only
    { 2, false, 1u << 20, 2, 0, 4 },    { 2, false, 1u << 20, 2, 1, 1 },    { 2, false, 1u << 20, 2, 2, 2 },    { 2, false, 1u << 20, 2, 3, 3 },
    { 2, false, MiB128 + 2, 0, 1, 1 },
  };
  for (const Row& r : rows) {
    LaunchFacts f = f32_24();
    f.elem_bytes = r.elem; f.quad = r.quad; f.f32_general = false; f.stored_bytes = r.bytes; f.row_loads = r.row_loads;
    const LaunchPlan p = plan_launch(f, ov(r.k));
    CHECK(!p.error && p.am == r.am, "elem %d quad %d bytes %llu row_loads %d override %d: mode %d, expected %d", r.elem, (int)r.quad, r.bytes, r.row_loads, r.k, p.am, r.am);
  }
}

static void inplace_unshaded()
{
  // LDS-staged bricks: general f32, shading 0, no skipping, mode <= 1, the setting on, not sparse, not clipped
  struct Row { const char* what; bool f32, skipping, lds_staging, sparse, clip; int shading, k; bool pool; bool staged, clipped; };
  const Row rows[] = {
    { "everything holds", true, false, true, false, false, 0, -1, false, true, false },
    { "mode 1", true, false, true, false, false, 0, 1, false, true, false },
    { "mode 2", true, false, true, false, false, 0, 2, false, false, false },
    { "mode 3", true, false, true, false, false, 0, 3, false, false, false },
    { "the setting off", true, false, false, false, false, 0, -1, false, false, false },
    { "skipping", true, true, true, false, false, 0, -1, false, false, false },
    { "sparse", true, false, true, true, false, 0, -1, false, false, false },
    { "clipped", true, false, true, false, true, 0, -1, false, false, true },
    { "clipped, the setting off", true, false, false, false, true, 0, -1, false, false, true },
    { "clipped and skipping", true, true, true, false, true, 0, -1, false, false, true },
    { "another layout", false, false, true, false, false, 0, -1, false, false, false },
    { "a pool without shading: in place all the same", true, false, true, false, false, 0, -1, true, true, false },
  };
  for (const Row& r : rows) {
    LaunchFacts f = f32_24();
    f.f32_general = r.f32; f.skipping = r.skipping; f.lds_staging = r.lds_staging; f.sparse = r.sparse; f.clip_on = r.clip; f.shading = r.shading; f.pool = r.pool;
    f.reference_material = false; // (unshaded: the material never matters)
    const LaunchPlan p = plan_launch(f, ov(r.k));
    CHECK(!p.error && !p.pooled && p.shading == 0 && p.skip == r.skipping, "%s: pooled %d shading %d skip %d", r.what, (int)p.pooled, p.shading, (int)p.skip);
    CHECK(p.march.lds_staged == r.staged && p.march.clipped == r.clipped && !p.march.material && !p.march.deep, "%s: staged %d clipped %d material %d deep %d", r.what,
          (int)p.march.lds_staged, (int)p.march.clipped, (int)p.march.material, (int)p.march.deep);
  }
  // the LDS of the 24^3 f32 volume under the 256 / 256 transfer function, by hand from the launcher's expressions:
  //   TF         256 x 16 + 256 x 4 + 32                                = 5152
  //   tables     4 x ((24 + 24 + 3) + (24 + 2)) = 308, rounded up to 16 = 320
  //   queues     kWaves x QCAP(shading 0) x 32 = 4 x 0 x 32             = 0
  //   march      max(5152 + 320 + 0, kWaves x 8 counters x 4 = 128)     = 5472
  //   staged     bricks at (5472 + 15) & ~15 = 5472; 5472 + 384 x 128 + sizeof(LdsRegion) 32 + 12 floats 48 + 2 ints 8 + 16 = 54728
  LaunchFacts f = f32_24();
  f.lds_staging = true;
  LaunchPlan p = plan_launch(f);
  CHECK(p.march.lds_staged && p.lds_brick_offset == 5472u && p.march_lds_bytes == 54728u, "staged: offset %u, %zu bytes", p.lds_brick_offset, p.march_lds_bytes);
  f.lds_staging = false;
  p = plan_launch(f);
  CHECK(!p.march.lds_staged && p.lds_brick_offset == 0u && p.march_lds_bytes == 5472u, "not staged: offset %u, %zu bytes", p.lds_brick_offset, p.march_lds_bytes);
  // 23 x 24 x 24: tables 4 x (50 + 26) = 304 -> 304 (a multiple of 16), TF + tables = 5456; mode 3: no tables, 5152 -> bricks at 5152
  f.nx = 23;
  CHECK(plan_launch(f).march_lds_bytes == 5456u, "23 x 24 x 24: %zu bytes", plan_launch(f).march_lds_bytes);
  CHECK(plan_launch(f, ov(3)).march_lds_bytes == 5152u, "mode 3: %zu bytes", plan_launch(f, ov(3)).march_lds_bytes);
  // mode 2: 8 x 26 + 4 x 50 = 408 -> 416
  CHECK(plan_launch(f, ov(2)).march_lds_bytes == 5152u + 416u, "mode 2: %zu bytes", plan_launch(f, ov(2)).march_lds_bytes);
}

static void inplace_shaded()
{
  for (int shading = 1; shading <= 2; ++shading) {
    struct Row { bool reference, clip, skipping; bool material, clipped; };
    const Row rows[] = { { true, false, false, false, false }, { false, false, false, true, false }, { true, true, false, true, true }, { false, true, false, true, true },
                         { true, false, true, false, false },  { false, false, true, true, false },  { true, true, true, true, true } };
    for (const Row& r : rows) {
      LaunchFacts f = f32_24();
      f.shading = shading; f.reference_material = r.reference; f.clip_on = r.clip; f.skipping = r.skipping; f.lds_staging = true;
      const LaunchPlan p = plan_launch(f);
      CHECK(!p.error && !p.pooled && p.shading == shading && p.skip == r.skipping, "shading %d: pooled %d shading %d", shading, (int)p.pooled, p.shading);
      CHECK(p.march.material == r.material && p.march.clipped == r.clipped && !p.march.lds_staged && !p.march.deep, "shading %d reference %d clip %d: material %d clipped %d",
            shading, (int)r.reference, (int)r.clip, (int)p.march.material, (int)p.march.clipped);
      // TF 5152 + tables 320 + queues 4 x 256 x 32 = 32768
      CHECK(p.march_lds_bytes == 38240u && p.lds_brick_offset == 0u, "shading %d: %zu bytes", shading, p.march_lds_bytes);
    }
  }
  LaunchFacts f = f32_24();
  f.shading = 7; // (anything but 0 and 1 is the full shading)
  CHECK(plan_launch(f).shading == 2, "shading 7 -> %d", plan_launch(f).shading);
}

static void pooled()
{
  for (int shading = 1; shading <= 2; ++shading) {
    struct Row { bool reference, clip, skipping, order; bool shade_material, shade_clipped; };
    const Row rows[] = {
      { true, false, false, true, false, false }, { false, false, false, true, true, false }, { true, false, true, false, false, false }, { false, false, true, true, true, false },
      // clipped: the march always, the shade kernel where it marches shadow rays (shading 2) - on the material variant whatever the material
      { true, true, false, true, shading == 2, shading == 2 }, { false, true, false, true, true, shading == 2 }, { true, true, true, true, shading == 2, shading == 2 },
    };
    for (const Row& r : rows) {
      LaunchFacts f = f32_24();
      f.shading = shading; f.pool = true; f.reference_material = r.reference; f.clip_on = r.clip; f.skipping = r.skipping; f.shade_order = r.order;
      const LaunchPlan p = plan_launch(f);
      CHECK(!p.error && p.pooled && p.shading == shading && p.skip == r.skipping, "shading %d: pooled %d", shading, (int)p.pooled);
      CHECK(!p.march.material && p.march.clipped == r.clip && !p.march.lds_staged && !p.march.deep, "shading %d clip %d: march material %d clipped %d deep %d", shading, (int)r.clip,
            (int)p.march.material, (int)p.march.clipped, (int)p.march.deep);
      CHECK(p.shade.material == r.shade_material && p.shade.clipped == r.shade_clipped, "shading %d reference %d clip %d: shade material %d clipped %d", shading, (int)r.reference,
            (int)r.clip, (int)p.shade.material, (int)p.shade.clipped);
      CHECK(p.shade_order == (shading == 2 && r.order), "shading %d order %d: shade_order %d", shading, (int)r.order, (int)p.shade_order);
      // march: queues 4 x 128 x 32 = 16384 + tables 320 + alpha 256 x 4 + 64 = 17792; shade: max(TF 5152 + tables 320, 64) = 5472
      CHECK(p.march_lds_bytes == 17792u && p.shade_lds_bytes == 5472u && p.lds_brick_offset == 0u, "shading %d: %zu / %zu bytes", shading, p.march_lds_bytes, p.shade_lds_bytes);
    }
  }
}

static void deep_rounds()
{
  struct Row { const char* what; int world; unsigned owned; bool sparse; u64 hint; bool skipping, clip; int elem, row_loads, k, deep_override; bool deep; };
  const Row rows[] = {
    { "one renderer", 1, 96, false, 0, false, false, 4, 0, -1, -1, false },
    { "a shard of 10000 blocks", 2, 10000, false, 0, false, false, 4, 0, -1, -1, true },
    { "a shard of 10001 blocks", 2, 10001, false, 0, false, false, 4, 0, -1, -1, false },
    { "sparse, 640000 pixels", 1, 96, true, 640000, false, false, 4, 0, -1, -1, true },
    { "sparse, 640001 pixels", 1, 96, true, 640001, false, false, 4, 0, -1, -1, false },
    { "sparse, no hint", 1, 96, true, 0, false, false, 4, 0, -1, -1, false },
    { "sparse in a shard", 2, 96, true, 1000, false, false, 4, 0, -1, -1, false },
    { "a shard, skipping", 2, 96, false, 0, true, false, 4, 0, -1, -1, false },
    { "a shard, clipped", 2, 96, false, 0, false, true, 4, 0, -1, -1, false },
    { "a shard, mode 1", 2, 96, false, 0, false, false, 4, 0, 1, -1, true },
    { "a shard, mode 2", 2, 96, false, 0, false, false, 4, 0, 2, -1, false },
    { "a shard, mode 3", 2, 96, false, 0, false, false, 4, 0, 3, -1, false },
    { "a shard, mode 4", 2, 96, false, 0, false, false, 2, 2, -1, -1, true },
    { "forced on", 1, 96, false, 0, false, false, 4, 0, -1, 1, true },
    { "forced off", 2, 96, false, 0, false, false, 4, 0, -1, 0, false },
    { "forced on, skipping", 1, 96, false, 0, true, false, 4, 0, -1, 1, false },
    { "forced on, clipped", 1, 96, false, 0, false, true, 4, 0, -1, 1, false },
    { "forced on, mode 2", 1, 96, false, 0, false, false, 4, 0, 2, 1, false },
    { "forced on, mode 4", 1, 96, false, 0, false, false, 2, 2, -1, 1, true },
  };
  for (int shading = 1; shading <= 2; ++shading)
    for (const Row& r : rows) {
      LaunchFacts f = f32_24();
      f.shading = shading; f.pool = true; f.world = r.world; f.n_blocks_owned = r.owned; f.sparse = r.sparse; f.sparse_hint_pixels = r.hint; f.skipping = r.skipping;
      f.clip_on = r.clip; f.elem_bytes = r.elem; f.f32_general = r.elem == 4; f.row_loads = r.row_loads;
      const LaunchPlan p = plan_launch(f, ov(r.k, r.deep_override));
      CHECK(!p.error && p.pooled && p.march.deep == r.deep, "%s (shading %d): deep %d, expected %d", r.what, shading, (int)p.march.deep, (int)r.deep);
      f.pool = false; // in place: never
      CHECK(!plan_launch(f, ov(r.k, r.deep_override)).march.deep, "%s in place: deep", r.what);
    }
}

static void shade_grid()
{
  struct Row { int setting, forced, blocks; };
  const Row rows[] = { { 0, 0, 1024 }, { 768, 0, 768 }, { 4096, 0, 1024 }, { -3, 0, 1024 }, { 768, 512, 512 }, { 0, 2000, 1024 }, { 768, -1, 768 } };
  for (const Row& r : rows) {
    LaunchFacts f = f32_24();
    f.shading = 2; f.pool = true; f.shade_blocks = r.setting;
    const LaunchPlan p = plan_launch(f, ov(-1, -1, r.forced));
    CHECK(p.shade_grid_blocks == r.blocks, "setting %d forced %d: %d blocks, expected %d", r.setting, r.forced, p.shade_grid_blocks, r.blocks);
  }
}

static void errors()
{
  LaunchFacts f = f32_24();
  CHECK(!plan_launch(f).error, "the plain frame is an error");
  // the transfer function: 16 n_color + 4 n_alpha + 32 <= 98304.  4096 / 8184: 65536 + 32736 + 32 = 98304; one more alpha entry does not fit
  f.n_color = 4096; f.n_alpha = 8184;
  CHECK(!plan_launch(f).error && tf_lds_bytes(4096, 8184) == 98304u, "a TF of 96 KiB is an error");
  f.n_alpha = 8185;
  CHECK(plan_launch(f).error && plan_launch(f, ov(3)).error && tf_lds_bytes(4096, 8185) == 0u, "a TF past 96 KiB is no error");
  f = f32_24();
  f.schedule = false;
  CHECK(plan_launch(f).error, "a dense frame with blocks and no schedule is no error");
  f.n_schedule = 0;
  CHECK(!plan_launch(f).error, "a dense frame without blocks is an error");
  f.n_schedule = 96; f.sparse = true;
  CHECK(!plan_launch(f).error, "a sparse frame needs no schedule");
  f = f32_24();
  f.tables = false;
  CHECK(plan_launch(f).error && !plan_launch(f, ov(3)).error, "tables are read below mode 3 alone");
}

// the launcher as it was nested, restated on the facts: which kernel it would have launched.  (am: the mode after the override and the row loads)
struct Launched { bool pooled, lds_staged, deep, material, clipped, shade_material, shade_clipped, order; };
static Launched launcher_as_it_was(const LaunchFacts& f, const LaunchOverrides& o, int shade, int am)
{
  Launched l = {};
  l.pooled = shade != 0 && f.pool;
  if (!l.pooled) {
    if (f.f32_general && shade == 0 && am <= 1 && !f.skipping && f.lds_staging && !f.sparse && !f.clip_on) { l.lds_staged = true; return l; }
    if (f.clip_on) { l.clipped = true; l.material = shade != 0; }
    else if (shade != 0 && !f.reference_material) l.material = true;
    return l;
  }
  l.order = shade == 2 && f.shade_order;
  if (!f.skipping && (am <= 1 || am == 4)) {
    bool deep = f.sparse ? f.world == 1 && f.sparse_hint_pixels > 0 && f.sparse_hint_pixels <= 640000 : f.world > 1 && f.n_blocks_owned <= 10000;
    if (o.deep >= 0) deep = o.deep != 0;
    if (deep && !f.clip_on) l.deep = true;
  }
  if (!l.deep) l.clipped = f.clip_on;
  l.shade_material = !f.reference_material;
  if (shade == 2 && f.clip_on) l.shade_material = l.shade_clipped = true;
  return l;
}

static void sweep()
{
  // every boolean fact x shading x the five addressing outcomes x the three element sizes x quad (x the deep override, the shard, the sparse hint)
  // (general: the layout is the general one - f32_general is that at 4 bytes a voxel, the only combination in which the fact can hold)
  long plans = 0, errors_seen = 0, variants[2] = { 0, 0 };
  for (int bits = 0; bits < (1 << 10); ++bits)
    for (int shading = 0; shading <= 2; ++shading)
      for (int mode = 0; mode <= 4; ++mode)
        for (int elem = 1; elem <= 4; elem *= 2)
          for (int quad = 0; quad <= 1; ++quad)
            for (int deep = -1; deep <= 1; ++deep)
              for (int shard = 0; shard <= 1; ++shard) {
                LaunchFacts f = f32_24();
                f.tables = bits & 1; f.pool = bits & 2; f.skipping = bits & 4; f.sparse = bits & 8; f.clip_on = bits & 16; f.lds_staging = bits & 32;
                f.reference_material = bits & 64; f.shade_order = bits & 128; f.schedule = bits & 256;
                const bool general = bits & 512;
                f.elem_bytes = elem; f.quad = quad; f.f32_general = general && elem == 4 && !quad;
                f.shading = shading;
                f.world = shard ? 2 : 1; f.sparse_hint_pixels = shard ? 0 : 5000;
                // the five outcomes from the facts that give them (8-bit voxels past 4 GiB are past 2^32 elements too: their mode 1 is the override's)
                int expect_am = mode;
                if (mode == 1 && elem > 1) f.stored_bytes = GiB4 + 4;
                if (mode == 2) f.stored_bytes = elem == 1 ? GiB4 + 1 : (u64)elem * 0xffffffffull;
                if (mode == 3) { f.nx = 24000; f.n_color = f.n_alpha = 4096; }
                f.row_loads = mode == 4 ? 2 : 1;
                if (mode == 4 && (elem == 4 || quad)) expect_am = 0;
                const LaunchOverrides o = ov(mode == 1 && elem == 1 ? 1 : -1, deep);
                const LaunchPlan p = plan_launch(f, o);
                ++plans;
                const bool expect_error = ((mode == 4 ? 0 : mode) < 3 && !f.tables) || (!f.sparse && !f.schedule); // (the row loads are mode 0's: they read its tables)
                CHECK(p.error == expect_error, "bits %d shading %d mode %d elem %d quad %d: error %d, expected %d", bits, shading, mode, elem, quad, (int)p.error, (int)expect_error);
                if (p.error) { ++errors_seen; continue; }
                CHECK(p.am == expect_am, "bits %d mode %d elem %d quad %d: mode %d", bits, mode, elem, quad, p.am);
                CHECK(march_variant_exists(p.shading, p.am, p.pooled, p.skip, p.march.lds_staged, p.march.deep, p.march.material, p.march.clipped, f.f32_general),
                      "bits %d shading %d mode %d elem %d quad %d deep %d shard %d: no such march variant", bits, shading, mode, elem, quad, deep, shard);
                CHECK(p.am != 4 || (elem <= 2 && !quad), "bits %d elem %d quad %d: row loads", bits, elem, quad);
                if (p.pooled)
                  CHECK(shade_variant_exists(p.shading, p.am, p.skip, p.shade.material, p.shade.clipped), "bits %d shading %d mode %d: no such shade variant", bits, shading, mode);
                const Launched l = launcher_as_it_was(f, o, shading, expect_am);
                CHECK(p.pooled == l.pooled && p.skip == f.skipping && p.march.lds_staged == l.lds_staged && p.march.deep == l.deep && p.march.material == l.material
                        && p.march.clipped == l.clipped,
                      "bits %d shading %d mode %d elem %d quad %d deep %d shard %d: march pooled %d staged %d deep %d material %d clipped %d", bits, shading, mode, elem, quad, deep, shard,
                      (int)p.pooled, (int)p.march.lds_staged, (int)p.march.deep, (int)p.march.material, (int)p.march.clipped);
                if (p.pooled)
                  CHECK(p.shade.material == l.shade_material && p.shade.clipped == l.shade_clipped && p.shade_order == l.order, "bits %d shading %d: shade material %d clipped %d order %d",
                        bits, shading, (int)p.shade.material, (int)p.shade.clipped, (int)p.shade_order);
                ++variants[p.pooled ? 1 : 0];
              }
  printf("sweep: %ld plans, %ld errors, %ld in place, %ld pooled\n", plans, errors_seen, variants[0], variants[1]);
  CHECK(plans == 1024L * 3 * 5 * 3 * 2 * 3 * 2 && variants[0] > 0 && variants[1] > 0 && errors_seen > 0, "the sweep's size");
  // and the two predicates against the combinations the kernels' own static_asserts named, as they were: nothing the launcher referenced is refused
  CHECK(!march_variant_exists(1, 0, true, false, false, false, true, false, true), "a pooled material march exists");
  CHECK(!march_variant_exists(0, 0, true, false, false, false, false, false, true), "an unshaded pooled march exists");
  CHECK(!march_variant_exists(0, 2, false, false, true, false, false, false, true), "LDS-staged bricks at mode 2 exist");
  CHECK(!march_variant_exists(0, 0, false, false, true, false, false, false, false), "LDS-staged bricks of another layout exist");
  CHECK(!march_variant_exists(1, 0, true, true, false, true, false, false, true), "a deep skipping march exists");
  CHECK(!march_variant_exists(1, 2, true, false, false, true, false, false, true), "a deep march at mode 2 exists");
  CHECK(!march_variant_exists(1, 0, false, false, false, false, false, true, true), "a clipped shading march without the material exists");
  CHECK(!march_variant_exists(0, 0, false, false, false, false, true, true, true), "a clipped unshaded march with the material exists");
  CHECK(!shade_variant_exists(1, 0, false, true, true), "a clipped shade kernel without shadow rays exists");
  CHECK(!shade_variant_exists(2, 0, false, false, true), "a clipped shade kernel without the material exists");
  CHECK(!shade_variant_exists(0, 0, false, false, false), "an unshaded shade kernel exists");
}

struct Scenario { const char* name; void (*run)(); };
static const Scenario kScenarios[] = { { "addressing", addressing }, { "row_loads", row_loads }, { "inplace_unshaded", inplace_unshaded }, { "inplace_shaded", inplace_shaded },
                                       { "pooled", pooled }, { "deep_rounds", deep_rounds }, { "shade_grid", shade_grid }, { "errors", errors }, { "sweep", sweep } };

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const Scenario& s : kScenarios) printf("%s\n", s.name);
    return 0;
  }
  for (const Scenario& s : kScenarios)
    if (argc == 2 && !strcmp(argv[1], s.name)) {
      s.run();
      printf("%s: %s\n", s.name, g_failed ? "FAILED" : "ok");
      return g_failed ? 1 : 0;
    }
  printf("usage: driver --list | <scenario>\n");
  return 2;
}
