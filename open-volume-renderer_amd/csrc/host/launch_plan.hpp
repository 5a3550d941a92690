// launch_plan.hpp - which march and shade kernel a frame takes and what each launch needs, as a pure function of a few facts about the frame:
// the ONLY statement of the variant rules.  Nothing here calls HIP or knows RayMarchParams: plan_raymarch (ovr_hip_kernels.hip) fills the facts
// and reads the environment switches, plan_kernels (ovr_hip_kernels.hip) turns a plan into its kernels - a switch over frame_kind to the lookup of the kind's
// device header, frame_kernels<VT> (ovr_hip_device.h) for the march -, launch_raymarch launches them, launch_ray_query the known-answer twin of a kind's kernel
// (ray_query.hpp), the kernels' static_asserts ask march_variant_exists / shade_variant_exists - and tests/test_launch_plan.py drives the same code on a
// machine without a GPU.  Every variant of the march renders the same frame bit for bit, so a wrong choice here shows as speed alone: hence the tables of that test.
// committed_frame is the ONLY statement of which committed state is drawn, frame_kind the only reading of a plan's kind (tests/test_ray_query_table.py).
#pragma once

#include "depth_output_host.hpp"
#include "gradient_opacity_host.hpp"
#include "max_depth_host.hpp"
#include "preintegration_host.hpp"

#include <algorithm>
#include <cstddef>

namespace ovrhip {

// ---- the sizes the decision needs (the device code includes this header for them)
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int request_queue_entries(int shade, bool pooled) { return shade == 0 ? 0 : (pooled ? 128 : 256); } // per wave; pooled: spills after every instruction
template <int SHADE, bool POOLED> struct QCfg {
  static constexpr int K = POOLED ? 4 : (SHADE == 0 ? 4 : 3);   // instructions (x4 steps) per round
  static constexpr int QCAP = request_queue_entries(SHADE, POOLED);
};
constexpr int kShadeReqBytes = 32;                      // sizeof(ShadeReq)
constexpr int kLdsBrickCap = 384;                       // LDS-staged bricks: 48 KiB of bricks per workgroup, two workgroups per CU
constexpr int kLdsRegionBytes = 32;                     // sizeof(LdsRegion)
constexpr int kShadeBlocks = 1024; // persistent shade grid: at most 4 workgroups per CU (size of the shade_counters workspace)
// The deep variant of the pooled march (6 instead of 4 instructions per round, 2 instead of 3 waves per SIMD) pays when the launch is
// bound by its longest ray's chain of dependent rounds rather than by throughput: image shards with few blocks.  Measured
// (profiles/r02_ab/r02b_deep.txt, march ms plain -> deep): C3 4-way 0.443 -> 0.422, 8-way 0.288 -> 0.254, 2-way (16 200 blocks) equal;
// but C5 (4K: 16 200 blocks even 8-way, throughput-bound) 0.508 -> 0.607 and C4 8-way (64-bit addressing) 0.604 -> 0.632: so only
// shards of at most 10 000 blocks with 32-bit addressing take it.
constexpr unsigned int kDeepMaxBlocks = 10000;
// ovr_hip_kernels.h's kBlockCounters and axis_a / b / z_entries, restated (that header needs the HIP runtime); ovr_hip_kernels.hip asserts that they agree
constexpr int kCounterWords = 8;
constexpr int kAxisAbExtra = 3, kAxisZExtra = 2; // table entries beyond nx + ny (a: n + 1, b: n + 2, whichever of x / y is the pair axis) and beyond nz

// ---- which instantiations exist: raymarch_kernel<VT, shade, am, pooled, skip, lds_staged, deep, material, clipped, cached> (f32_general: VT is the general f32
// layout) and shade_pool_kernel<VT, shade, am, skip, material, clipped, cached>; am == 4 only for the layouts row_load_layout names.
// cached (the shadow cache): the shadow term is one tap into a lattice instead of a march - on the kernels that shade without a
// shadow march (shade 1), riding on the material variant like the clipped ones; the pooled march does not shade and has no cached twin
// orthographic (the orthographic camera): a per-lane ray origin and the miss rule of primary_box_test.  THE ORTHOGRAPHIC VARIANTS EXIST
// EXACTLY WHERE THE CLIPPED ONES EXIST, as the clipped ones ride on the material variants: an orthographic frame without a clip box runs them with the unit
// box (whose bounds give the unclipped test's bits), and it never takes the LDS-staged or the deep march - a clipped frame takes neither
constexpr bool row_load_layout(int elem_bytes, bool quad) { return elem_bytes <= 2 && !quad; } // the 16-bit pairs (and 8-bit ones) as aligned 8-byte rows
constexpr bool march_variant_exists(int shade, int am, bool pooled, bool skip, bool lds_staged, bool deep, bool material, bool clipped, bool f32_general,
                                    bool cached = false, bool orthographic = false)
{
  if (orthographic && (!clipped || lds_staged || deep)) return false;          // on the clipped variants alone
  if (cached && !(shade == 1 && material && !pooled)) return false;           // where the march shades, without a shadow march, on the material variant
  if (shade < 0 || shade > 2 || am < 0 || am > 4 || (f32_general && am == 4)) return false;
  if (pooled && shade == 0) return false;                                      // nothing to shade: the in-place march is the only pipeline
  if (lds_staged) return f32_general && shade == 0 && !skip && am <= 1 && !deep && !material && !clipped; // the unshaded in-place march only
  if (deep) return pooled && !skip && (am <= 1 || am == 4) && !material && !clipped; // the plain pooled march with 32-bit addressing
  if (material && (shade == 0 || pooled)) return false;                        // where the march shades: in place (pooled: shade_pool_kernel)
  if (clipped && !pooled && material != (shade != 0)) return false;            // the clipped in-place march rides on the material variant where it shades
  return true;
}
constexpr bool shade_variant_exists(int shade, int am, bool skip, bool material, bool clipped, bool cached = false, bool orthographic = false)
{
  if (shade < 1 || shade > 2 || am < 0 || am > 4) return false;
  // the shade kernel forms no primary ray: its orthographic twin differs by the view vector alone, so it rides on the material variant - the clipped one where
  // the kernel marches shadow rays (an orthographic frame is a clipped frame), the plain one where it does not
  if (orthographic && !(material && clipped == (shade == 2))) return false;
  if (cached && !(shade == 1 && material)) return false;
  (void)skip;
  return !clipped || (shade == 2 && material); // clipped where the shade kernel marches shadow rays, on the material variant
}

// project_kernel<VT, am, mode, skip, clipped> (open-volume-renderer_amd/projection.py is the arithmetic): the projections of the general
// layouts - mode 1 maximum, 2 minimum, 3 mean (include/ovr_hip.h OVR_HIP_PROJECT_*).  skip: the range-skipping twin, which only an extremum has (a mean needs
// every sample); am == 4 only for the layouts row_load_layout names, like the march
constexpr int kProjectMaximum = 1, kProjectMinimum = 2, kProjectMean = 3;
constexpr int kProjectK = 4; // instructions (x 4 steps) per round, the unshaded march's
constexpr bool project_variant_exists(int mode, int am, bool skip, bool clipped, bool orthographic = false)
{
  if (orthographic && !clipped) return false; // both box tests exist for every variant, the orthographic camera on the clipped one
  if (mode < kProjectMaximum || mode > kProjectMean || am < 0 || am > 4) return false;
  return !skip || mode != kProjectMean;
}

// isosurface_kernel<VT, am, shade, skip, clipped> (open-volume-renderer_amd/isosurface.py is the arithmetic): opaque level sets of the general
// layouts for up to kMaxIsovalues isovalues.  shade: the committed shading mode (0 colour alone, 1 gradient-shaded, 2 with the hard shadow walk); skip: the
// range-skipping twin, which every shading mode has (primary and shadow walk skip alike); the material is a run-time argument, not a variant
constexpr int kMaxIsovalues = 4; // include/ovr_hip.h OVR_HIP_MAX_ISOVALUES
// translucent: every crossing composited with its isovalue's opacity - like the orthographic twins ON THE CLIPPED VARIANTS ALONE (a frame
// without a clip box runs them with the unit box, whose bounds give the unclipped test's bits), for both cameras
// ao (ambient occlusion): K hemisphere walks per event scale the ambient term - twins of the TRANSLUCENT kernels alone (an opaque frame runs
// them with its all-ones opacities, section 19's identity), under a shading mode that has an ambient term
// context (open-volume-renderer_amd/isosurface_context.py): isosurface_context_kernel<VT, am, shade, orthographic>, the unshaded march
// composited around the translucent walk's events - on the clipped variants alone like the translucent twins, for both cameras and the three shading modes; it
// fetches every step (no skipping twin) and casts no ambient occlusion (no AO twin)
constexpr bool isosurface_variant_exists(int shade, int am, bool skip, bool clipped, bool orthographic = false, bool translucent = false, bool ao = false, bool context = false)
{
  if (context) return clipped && !skip && !ao && translucent && shade >= 0 && shade <= 2 && am >= 0 && am <= 4;
  (void)skip; // both walks and both box tests exist for every variant, the orthographic camera on the clipped test
  if ((orthographic || translucent) && !clipped) return false;
  if (ao && !(translucent && shade >= 1)) return false;
  return shade >= 0 && shade <= 2 && am >= 0 && am <= 4;
}

// slice_plane_kernel<VT, am, clipped> and slice_walk_kernel<VT, am, skip, clipped> (open-volume-renderer_amd/slices.py is the arithmetic): cut
// planes and thick slabs of the general layouts, up to kMaxSlices of them.  walks: a slab is among the committed slices - the projection's walk on the slab's
// interval, the winning slice's mode a run-time value; without one the plane kernel, one lane per ray, which has nothing to skip.  The orthographic twins exist
// on the clipped kernels alone, under the rule the projection's follow
constexpr int kMaxSlices = 4; // include/ovr_hip.h OVR_HIP_MAX_SLICES
// context (open-volume-renderer_amd/slice_context.py): slice_context_kernel<VT, am, orthographic>, the unshaded march in front of the winning
// slice - ONE kernel for plane-only and slab sets alike (`walks` is not read), like the translucent isosurface twins ON THE CLIPPED VARIANTS ALONE (a frame
// without a clip box runs it with the unit box), for both cameras; it fetches every step: no skipping twin
constexpr bool slice_variant_exists(bool walks, int am, bool skip, bool clipped, bool orthographic = false, bool context = false)
{
  if (context) return clipped && !skip && am >= 0 && am <= 4;
  if (orthographic && !clipped) return false;
  if (skip && !walks) return false; // one tap per ray: no fetch to drop
  return am >= 0 && am <= 4;
}

// preintegrated_kernel<VT, am, orthographic> (open-volume-renderer_amd/preintegration.py is the arithmetic): the unshaded march with
// every SEGMENT between two consecutive samples classified by the transfer function's integral over the values it spans - like the context kernels ON THE
// CLIPPED VARIANTS ALONE (a frame without a clip box runs it with the unit box), for both cameras, of the general layouts; it fetches every step: no skipping twin
constexpr bool preintegrated_variant_exists(int am, bool skip, bool clipped, bool orthographic = false)
{
  (void)orthographic; // both cameras
  return clipped && !skip && am >= 0 && am <= 4;
}

// gradient_opacity_kernel<VT, am, shade, orthographic> (open-volume-renderer_amd/gradient_opacity.py is the arithmetic): the march with
// every sample's table opacity weighted by a ramp over the gradient's magnitude - like the context kernels ON THE CLIPPED VARIANTS ALONE (a frame without a clip
// box runs it with the unit box), for shading NONE and GRADIENT and both cameras, of the general layouts; it fetches every step: no skipping twin
constexpr bool gradient_opacity_variant_exists(int shade, int am, bool skip, bool clipped, bool orthographic = false)
{
  (void)orthographic; // both cameras
  return (shade == 0 || shade == 1) && clipped && !skip && am >= 0 && am <= 4;
}

// max_depth_kernel<VT, am, shade, orthographic> (open-volume-renderer_amd/max_depth.py is the arithmetic): the march that ends on a
// per-pixel ray parameter the caller hands in - like the context kernels ON THE CLIPPED VARIANTS ALONE (a frame without a clip box runs it with the unit box),
// for shading NONE and GRADIENT and both cameras, of the general layouts; it fetches every step: no skipping twin
constexpr bool max_depth_variant_exists(int shade, int am, bool skip, bool clipped, bool orthographic = false)
{
  (void)orthographic; // both cameras
  return (shade == 0 || shade == 1) && clipped && !skip && am >= 0 && am <= 4;
}

// depth_output_kernel<VT, am, shade, orthographic> (open-volume-renderer_amd/depth_output.py is the arithmetic): the march that also
// writes where along each ray it became opaque - the depth-limited kernel's variants exactly: ON THE CLIPPED VARIANTS ALONE, for shading NONE and GRADIENT and
// both cameras, of the general layouts; it fetches every step: no skipping twin
constexpr bool depth_output_variant_exists(int shade, int am, bool skip, bool clipped, bool orthographic = false)
{
  return max_depth_variant_exists(shade, am, skip, clipped, orthographic);
}

// ---- LDS arithmetic
// the transfer function always lives in LDS; 0 = does not fit next to the request queues (the frame is an error)
// (+ 32: both tables carry one more entry, a copy of their last one - stage_tf)
constexpr size_t tf_lds_bytes(int n_color, int n_alpha)
{
  const size_t need = (size_t)n_color * 16 + (size_t)n_alpha * 4 + 32;
  return need <= 96 * 1024 ? need : 0;
}
// the per-axis offset tables as the kernels stage them (stage_tables): modes 0 / 1 / 4 hold 32-bit entries, 2 a 64-bit z table, 3 none
constexpr size_t axis_table_bytes(int nx, int ny, int nz, int am)
{
  const size_t ab = (size_t)(nx + ny + kAxisAbExtra), ez = (size_t)(nz + kAxisZExtra);
  return am == 3 ? 0 : am == 2 ? ez * 8 + ab * 4 : (ab + ez) * 4;
}
constexpr size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
// the LDS budget of a pre-integrated frame's workgroup - axis tables + transfer function + the 16 * (M + 1) bytes of the node table: a third of a CU's 160 KiB
// (a multiple of 16), so that three workgroups - one wave each per SIMD, the march's kMarchWavesPerEu = 3 - stay resident.  The kernel is gather-bound like the
// march: a table that cost it the third wave would cost more than its finer nodes gain, so the subdivision S gives way first (4, 2, 1) and a transfer function
// whose S = 1 table does not fit is refused, as one whose tables exceed tf_lds_bytes' bound is
constexpr size_t kPreintegrationLdsBudget = ((size_t)160 * 1024 / 3) & ~(size_t)15;

// Addressing mode of a volume layout: 0 = 32-bit byte offsets (<= 4 GiB), 1 = 32-bit element offsets (< 2^32 stored voxels), 2 = 64-bit z
// table, 3 = computed 64-bit offsets, no tables.  Modes 0-2 keep the per-axis tables in LDS next to the transfer function and the request
// queues (32 KiB in the in-place march): a volume with one very long axis - small in bytes, tens of thousands of voxels long - whose
// tables do not fit in the 160 KiB of a CU takes mode 3 whatever its size.
constexpr int addressing_mode(unsigned long long stored_bytes, int elem_bytes, int nx, int ny, int nz, int n_color, int n_alpha)
{
  const int am = stored_bytes <= 0x100000000ull ? 0 : (stored_bytes / (unsigned long long)elem_bytes < 0xffffffffull) ? 1 : 2;
  const size_t tables = axis_table_bytes(nx, ny, nz, am);
  const size_t fixed = tf_lds_bytes(n_color, n_alpha) + (size_t)kWaves * request_queue_entries(1, false) * kShadeReqBytes + 1024; // TF + the largest request queues + slack
  return ((am == 2 && tables > 64 * 1024) || tables + 16 + fixed > 160 * 1024) ? 3 : am;
}

// ---- the kind of a frame
// What is committed decides what is drawn, and THIS is the precedence: slices over isovalues over a projection mode over the march.  Committed state of a lower
// rank is kept and not drawn - and not read: the isosurface context, the ambient occlusion and the opacities mean nothing under slices.  plan_launch, the
// `active` fields of the getters (ovr_hip_api.cpp) and the frame's layout and skipping steps (host/frame.cpp) all ask here
enum class CommittedFrame { March, Projection, Isovalues, Slices };
constexpr CommittedFrame committed_frame(int slices, int isovalues, int projection)
{
  return slices != 0 ? CommittedFrame::Slices : isovalues != 0 ? CommittedFrame::Isovalues : projection != 0 ? CommittedFrame::Projection : CommittedFrame::March;
}
static_assert(committed_frame(1, 1, 1) == CommittedFrame::Slices && committed_frame(0, 1, 1) == CommittedFrame::Isovalues && committed_frame(0, 0, 1) == CommittedFrame::Projection
                && committed_frame(0, 0, 0) == CommittedFrame::March,
              "slices over isovalues over projection over march");
// one value per kernel family that can stand in the march's place (frame_kind below reads it off a plan)
enum class FrameKind { March, Projection, Isosurface, IsosurfaceLayers, IsosurfaceAo, IsosurfaceContext, SlicePlane, SliceWalk, SliceContext, PreintegratedMarch, GradientOpacityMarch, DepthLimitedMarch, DepthOutputMarch };

// ---- facts -> plan
struct LaunchFacts {
  int elem_bytes = 4;                 // of a stored voxel
  bool quad = false, f32_general = false;
  int nx = 1, ny = 1, nz = 1;
  unsigned long long stored_bytes = 0;
  bool tables = true;                 // the layout's axis tables are present
  int n_color = 1, n_alpha = 1, shading = 0;
  bool pool = false, skipping = false, sparse = false; // request pool / majorant grid / sample list present
  unsigned long long sparse_hint_pixels = 0;
  int world = 1;
  unsigned int n_blocks_owned = 0, n_schedule = 0;
  bool schedule = true;               // the dense frame's block list is present
  bool clip_on = false, lds_staging = false;
  int row_loads = 0;                  // 0 = by the layout's size, 1 = never, 2 = always
  int shade_blocks = 0;               // 0 = the default
  bool reference_material = true, shade_order = false; // the material is the reference's; the pool has an order buffer
  bool shadow_cache = false;          // a valid shadow lattice is bound (RayMarchParams::shadow_lattice): a frame with full shading reads it
  int projection = 0;                 // 0: the march; 1 ... 3: a projection frame (kProjectMaximum ...) - shading, pool, majorants and LDS staging are not read
  bool ranges = false;                // the macrocells' value ranges are bound (RayMarchParams::mc_ranges): an extremum may skip by them
  bool orthographic = false;          // the committed camera is orthographic (ovr_hip_set_camera_orthographic): the frame takes the orthographic twins of the clipped variants
  int isosurfaces = 0;                // the number of committed isovalues; > 0: an isosurface frame - `projection` is kept but not drawn, pool, majorants and LDS staging are not read
  bool translucent = false;           // one of the committed isovalues' opacities is below 1 (ovr_hip_set_isosurface_layers): an isosurface frame takes the translucent twins
  bool ambient_occlusion = false;     // ambient-occlusion samples are committed (ovr_hip_set_ambient_occlusion, K > 0): a shaded isosurface frame takes the AO twins
  int slices = 0;                     // the number of committed slices; > 0: a slice frame - `isosurfaces` and `projection` are kept but not drawn, shading, pool, majorants and LDS staging are not read
  bool slice_walks = false;           // one of the committed slices is a slab (thickness > 0): the frame takes the walk kernel
  bool slice_extremum = false;        // one of the committed slabs is a MAXIMUM or MINIMUM slab: the only ones range skipping drops fetches of
  bool slice_context = false;         // the slice context is committed in mode FRONT (ovr_hip_set_slice_context): a slice frame takes the context kernel - read only while slices > 0
  bool isosurface_context = false;    // the isosurface context is committed in mode VOLUME (ovr_hip_set_isosurface_context): an isosurface frame takes the context kernel - read only while isosurfaces > 0 (and slices == 0)
  bool preintegrated = false;         // pre-integration is committed in mode SEGMENTS (ovr_hip_set_preintegration): the unshaded march takes the pre-integrated kernel - read only while the committed frame is the march and shading == 0
  bool gradient_opacity = false;      // gradient opacity is committed in mode RAMP (ovr_hip_set_gradient_opacity): the march under shading NONE or GRADIENT takes the gradient-opacity kernel - read only while the committed frame is the march and the frame is not a pre-integrated one
  bool max_depth = false;             // a depth image of the framebuffer's size is committed (ovr_hip_set_max_depth): the march under shading NONE or GRADIENT takes the depth-limited kernel - read only while the committed frame is the march and neither pre-integration nor gradient opacity draws it
  bool depth_output = false;          // depth output is committed in mode ON (ovr_hip_set_depth_output): the march under shading NONE or GRADIENT takes the depth-output kernel, which applies the depth limit itself where max_depth is set - read only while the committed frame is the march and neither pre-integration nor gradient opacity draws it
  float depth_threshold = 0.f;        // its tau (the kernel reads RayMarchParams::depth_tau; the plan carries it for the record)
};
// the environment switches OVR_HIP_ADDRESSING / OVR_HIP_DEEP / OVR_HIP_SHADE_BLOCKS as data (diagnostics and measurements)
struct LaunchOverrides { int addressing = -1, deep = -1, shade_blocks = 0; };

struct LaunchPlan {
  int shading = 0;                    // 0, 1 or 2: the kernels' SHADE
  int am = 0;                         // 0 ... 3 above; 4 = mode 0 with the 16-bit pairs read as aligned 8-byte rows (RowLoads)
  bool pooled = false, skip = false;
  struct March { bool lds_staged = false, deep = false, material = false, clipped = false; } march;
  struct Shade { bool material = false, clipped = false; } shade;
  bool shade_order = false;           // the shade kernel meets the runs sorted by light beam (PoolDesc::order)
  bool orthographic = false;          // every kernel of the frame that forms a primary ray or a view vector is the orthographic twin (of the clipped variant)
  bool cached = false;                // the kernels that shade take the shadow term from the lattice: SHADE 1, material, no box test while shading
  // a projection frame (LaunchFacts::projection != 0): project_kernel in the march's place, nothing else of the plan but `am` is read
  // (lds_bytes, here and below: march_lds_bytes on such a frame and 0 on any other - the launches read march_lds_bytes, the plan tests pin both)
  struct Project { int mode = 0; bool skip = false, clipped = false; size_t lds_bytes = 0; } project;
  // an isosurface frame (LaunchFacts::isosurfaces > 0): isosurface_kernel in the march's place, nothing else of the plan but `am` and `shading` is read
  // (context: isosurface_context_kernel - the unshaded march around the level sets, with the transfer function in LDS behind the axis tables; translucent and
  // clipped are set, skip and ambient_occlusion never)
  struct Isosurface { bool on = false, skip = false, clipped = false; size_t lds_bytes = 0; bool translucent = false; bool context = false; } isosurface;
  size_t march_lds_bytes = 0, shade_lds_bytes = 0;
  unsigned int lds_brick_offset = 0;  // LDS-staged bricks: where they start, behind the tables and the TF
  int shade_grid_blocks = 0;
  bool error = false;                 // the frame cannot be launched (hipErrorInvalidValue)
  bool ambient_occlusion = false;     // an isosurface frame's kernel is the AO twin of the translucent one (isosurface.translucent and isosurface.clipped are set)
  // a slice frame (LaunchFacts::slices > 0): slice_plane_kernel or slice_walk_kernel in the march's place, nothing else of the plan but `am` is read
  // (context: slice_context_kernel - the unshaded march in front of the slices, with the transfer function in LDS behind the axis tables)
  struct Slices { bool on = false, walks = false, skip = false, clipped = false; size_t lds_bytes = 0; bool context = false; } slices;
  // a pre-integrated march (LaunchFacts::preintegrated on the unshaded march): preintegrated_kernel in the march's place, nothing else of the plan but `am` is
  // read.  LDS: [axis tables][transfer function][node table, 16-byte aligned]; subdivision / nodes: S and M of the node table the budget allows
  struct Preintegrated { bool on = false, clipped = false; size_t lds_bytes = 0; int subdivision = 0, nodes = 0; } preintegrated;
  // a gradient-opacity march (LaunchFacts::gradient_opacity on the march under shading NONE or GRADIENT): gradient_opacity_kernel in the march's place, nothing
  // else of the plan but `am` is read.  LDS: [axis tables][transfer function], the slice context's carve; shade: the GRADIENT-shaded kernel
  struct GradientOpacity { bool on = false, clipped = false, shade = false; size_t lds_bytes = 0; } gradient_opacity;
  // a depth-limited march (LaunchFacts::max_depth on the march under shading NONE or GRADIENT): max_depth_kernel in the march's place, nothing else of the plan
  // but `am` is read.  LDS: [axis tables][transfer function], the slice context's carve; shade: the GRADIENT-shaded kernel
  struct MaxDepth { bool on = false, clipped = false, shade = false; size_t lds_bytes = 0; } max_depth;
  // a depth-output march (LaunchFacts::depth_output on the march under shading NONE or GRADIENT): depth_output_kernel in the march's place, nothing else of the
  // plan but `am` is read.  LDS: the depth-limited march's carve; shade: the GRADIENT-shaded kernel; limited: a depth image is bound and the kernel loads it
  struct DepthOutput { bool on = false, clipped = false, shade = false, limited = false; size_t lds_bytes = 0; } depth_output;
};

// the deep rounds' rule without the kernel's own conditions
inline bool deep_rounds_pay(const LaunchFacts& f, const LaunchOverrides& o)
{
  if (o.deep >= 0) return o.deep != 0;
  // sparse (foveated) frames: the kept rays are few and concentrated where the rays are long - the same floor (march 1.12 -> 1.01 ms at the
  // app's default focus); the host passes the previous frame's pixel count, the list's length is only known on the device
  if (f.sparse) return f.world == 1 && f.sparse_hint_pixels > 0 && f.sparse_hint_pixels <= 64ull * kDeepMaxBlocks;
  // (the threshold was measured on the number of blocks a shard OWNS, launched or not)
  return f.world > 1 && f.n_blocks_owned <= kDeepMaxBlocks;
}

// the addressing step of every plan: the layout's mode, a more general one on request (OVR_HIP_ADDRESSING), then the row loads on mode 0 - mode 4: layouts the
// caches do not serve (by size), or forced either way.  error: the mode's tables or the dense frame's block list are missing
struct Addressing { int am; bool error; };
inline Addressing plan_addressing(const LaunchFacts& f, const LaunchOverrides& o)
{
  int am = addressing_mode(f.stored_bytes, f.elem_bytes, f.nx, f.ny, f.nz, f.n_color, f.n_alpha);
  if (o.addressing >= 0) am = std::min(std::max(am, o.addressing), 3);
  const bool error = (am < 3 && !f.tables) || (!f.sparse && f.n_schedule > 0 && !f.schedule);
  if (row_load_layout(f.elem_bytes, f.quad) && am == 0 && (f.row_loads > 0 ? f.row_loads != 1 : f.stored_bytes > (128ull << 20))) am = 4;
  return { am, error };
}

// what a projection and an isosurface frame share - the frames of the walk: one kernel of the general layout, in place, in the in-place march's place in the
// launch sequence (march_lds_bytes is its LDS).  The transfer function is read from global memory, once per ray: LDS holds the axis tables alone (and the counter
// reduction's words).  clipped: a clip box, or a twin that exists on the clipped variants alone - a frame without a clip box runs those with the unit box
struct WalkFrame { bool clipped; size_t lds_bytes; };
inline WalkFrame plan_walk_frame(LaunchPlan& pl, const LaunchFacts& f, int am, bool translucent = false)
{
  pl.am = am;
  pl.orthographic = f.orthographic;
  pl.march_lds_bytes = std::max<size_t>(align16(axis_table_bytes(f.nx, f.ny, f.nz, am)), (size_t)kWaves * kCounterWords * 4);
  return { f.clip_on || f.orthographic || translucent, pl.march_lds_bytes };
}

// a projection frame: the skipping twin where the ranges are bound and the mode is an extremum
inline LaunchPlan plan_projection(const LaunchFacts& f, const LaunchOverrides& o)
{
  LaunchPlan pl;
  const Addressing a = plan_addressing(f, o);
  if (a.error || f.projection < kProjectMaximum || f.projection > kProjectMean || f.quad) { pl.error = true; return pl; }
  const WalkFrame w = plan_walk_frame(pl, f, a.am);
  pl.project.mode = f.projection;
  pl.project.skip = f.ranges && f.projection != kProjectMean;
  pl.project.clipped = w.clipped;
  pl.project.lds_bytes = w.lds_bytes;
  return pl;
}

// an isosurface frame: the committed shading mode as the kernel's, the skipping twin whenever the ranges are bound
inline LaunchPlan plan_isosurface(const LaunchFacts& f, const LaunchOverrides& o)
{
  LaunchPlan pl;
  const Addressing a = plan_addressing(f, o);
  if (a.error || f.isosurfaces < 1 || f.isosurfaces > kMaxIsovalues || f.quad) { pl.error = true; return pl; }
  const int shading = f.shading == 0 || f.shading == 1 ? f.shading : 2;
  const bool ctx = f.isosurface_context;
  const bool ao = !ctx && f.ambient_occlusion && shading >= 1; // without an ambient term on the surface (or under the context) the committed samples are kept and not used
  WalkFrame w = plan_walk_frame(pl, f, a.am, f.translucent || ao || ctx);
  if (ctx) { // the march's classification per step: the transfer function in LDS behind the tables, as plan_slices has it under its context (0: it does not fit)
    const size_t tf = tf_lds_bytes(f.n_color, f.n_alpha);
    if (tf == 0) { pl = LaunchPlan(); pl.error = true; return pl; }
    w.lds_bytes = pl.march_lds_bytes = std::max<size_t>(align16(axis_table_bytes(f.nx, f.ny, f.nz, a.am)) + tf, (size_t)kWaves * kCounterWords * 4);
  }
  pl.shading = shading;
  pl.isosurface.on = true;
  pl.isosurface.context = ctx;
  pl.isosurface.skip = !ctx && f.ranges; // a context frame fetches every step, on the primary walk and on a shadow walk
  pl.isosurface.translucent = f.translucent || ao || ctx; // the AO twins and the context are the translucent path's: an opaque frame runs it with its all-ones opacities
  pl.ambient_occlusion = ao;
  pl.isosurface.clipped = w.clipped;
  pl.isosurface.lds_bytes = w.lds_bytes;
  return pl;
}

// a slice frame: the plane kernel while every slice is a plane, the walk kernel otherwise - its skipping twin where the ranges are bound and a slab is an
// extremum's (planes and MEAN slabs fetch everything: a frame of those alone keeps the plain kernel)
inline LaunchPlan plan_slices(const LaunchFacts& f, const LaunchOverrides& o)
{
  LaunchPlan pl;
  const Addressing a = plan_addressing(f, o);
  if (a.error || f.slices < 1 || f.slices > kMaxSlices || f.quad) { pl.error = true; return pl; }
  WalkFrame w = plan_walk_frame(pl, f, a.am, f.slice_context);
  if (f.slice_context) { // the march's classification per step: the transfer function in LDS behind the tables, as the march has it (0: it does not fit)
    const size_t tf = tf_lds_bytes(f.n_color, f.n_alpha);
    if (tf == 0) { pl = LaunchPlan(); pl.error = true; return pl; }
    w.lds_bytes = pl.march_lds_bytes = std::max<size_t>(align16(axis_table_bytes(f.nx, f.ny, f.nz, a.am)) + tf, (size_t)kWaves * kCounterWords * 4);
  }
  pl.slices.on = true;
  pl.slices.walks = f.slice_walks;
  pl.slices.context = f.slice_context;
  pl.slices.skip = !f.slice_context && f.slice_walks && f.slice_extremum && f.ranges; // a context frame fetches every step, a slab's included
  pl.slices.clipped = w.clipped;
  pl.slices.lds_bytes = w.lds_bytes;
  return pl;
}

// a pre-integrated march: one kernel of the general layout on the clipped box test, the transfer function and the node table in LDS behind the axis tables.
// error: the transfer function does not fit (tf_lds_bytes), or the node table of subdivision 1 does not fit the budget beside tables and transfer function
inline LaunchPlan plan_preintegrated(const LaunchFacts& f, const LaunchOverrides& o)
{
  LaunchPlan pl;
  const Addressing a = plan_addressing(f, o);
  const size_t tf = tf_lds_bytes(f.n_color, f.n_alpha);
  if (a.error || tf == 0 || f.quad) { pl.error = true; return pl; }
  const size_t front = align16(align16(axis_table_bytes(f.nx, f.ny, f.nz, a.am)) + tf); // where the node table starts
  const int s = front < kPreintegrationLdsBudget ? preintegration_subdivision(f.n_color, f.n_alpha, kPreintegrationLdsBudget - front) : 0;
  if (s == 0) { pl.error = true; return pl; }
  const WalkFrame w = plan_walk_frame(pl, f, a.am, true);
  pl.preintegrated.on = true;
  pl.preintegrated.clipped = w.clipped;
  pl.preintegrated.subdivision = s;
  pl.preintegrated.nodes = preintegration_nodes(f.n_color, f.n_alpha, s);
  pl.preintegrated.lds_bytes = pl.march_lds_bytes = std::max<size_t>(front + preintegration_table_bytes(pl.preintegrated.nodes), (size_t)kWaves * kCounterWords * 4);
  return pl;
}

// a gradient-opacity march: one kernel of the general layout on the clipped box test, the transfer function in LDS behind the axis tables.
// error: the transfer function does not fit (tf_lds_bytes)
inline LaunchPlan plan_gradient_opacity(const LaunchFacts& f, const LaunchOverrides& o)
{
  LaunchPlan pl;
  const Addressing a = plan_addressing(f, o);
  const size_t tf = tf_lds_bytes(f.n_color, f.n_alpha);
  if (a.error || tf == 0 || f.quad || !(f.shading == 0 || f.shading == 1)) { pl.error = true; return pl; }
  const WalkFrame w = plan_walk_frame(pl, f, a.am, true);
  pl.shading = f.shading;
  pl.gradient_opacity.on = true;
  pl.gradient_opacity.clipped = w.clipped;
  pl.gradient_opacity.shade = f.shading == 1;
  pl.gradient_opacity.lds_bytes = pl.march_lds_bytes = std::max<size_t>(align16(axis_table_bytes(f.nx, f.ny, f.nz, a.am)) + tf, (size_t)kWaves * kCounterWords * 4);
  return pl;
}

// a depth-limited march: one kernel of the general layout on the clipped box test, the transfer function in LDS behind the axis tables.
// error: the transfer function does not fit (tf_lds_bytes)
inline LaunchPlan plan_max_depth(const LaunchFacts& f, const LaunchOverrides& o)
{
  LaunchPlan pl;
  const Addressing a = plan_addressing(f, o);
  const size_t tf = tf_lds_bytes(f.n_color, f.n_alpha);
  if (a.error || tf == 0 || f.quad || !(f.shading == 0 || f.shading == 1)) { pl.error = true; return pl; }
  const WalkFrame w = plan_walk_frame(pl, f, a.am, true);
  pl.shading = f.shading;
  pl.max_depth.on = true;
  pl.max_depth.clipped = w.clipped;
  pl.max_depth.shade = f.shading == 1;
  pl.max_depth.lds_bytes = pl.march_lds_bytes = std::max<size_t>(align16(axis_table_bytes(f.nx, f.ny, f.nz, a.am)) + tf, (size_t)kWaves * kCounterWords * 4);
  return pl;
}

// a depth-output march: the depth-limited march's plan with the depth layer's kernel - one kernel of the general layout on the clipped box test, the transfer
// function in LDS behind the axis tables.  error: the transfer function does not fit (tf_lds_bytes)
inline LaunchPlan plan_depth_output(const LaunchFacts& f, const LaunchOverrides& o)
{
  LaunchPlan pl;
  const Addressing a = plan_addressing(f, o);
  const size_t tf = tf_lds_bytes(f.n_color, f.n_alpha);
  if (a.error || tf == 0 || f.quad || !(f.shading == 0 || f.shading == 1)) { pl.error = true; return pl; }
  const WalkFrame w = plan_walk_frame(pl, f, a.am, true);
  pl.shading = f.shading;
  pl.depth_output.on = true;
  pl.depth_output.clipped = w.clipped;
  pl.depth_output.shade = f.shading == 1;
  pl.depth_output.limited = f.max_depth;
  pl.depth_output.lds_bytes = pl.march_lds_bytes = std::max<size_t>(align16(axis_table_bytes(f.nx, f.ny, f.nz, a.am)) + tf, (size_t)kWaves * kCounterWords * 4);
  return pl;
}

inline LaunchPlan plan_launch(const LaunchFacts& f, const LaunchOverrides& o = LaunchOverrides())
{
  switch (committed_frame(f.slices, f.isosurfaces, f.projection)) {
  case CommittedFrame::Slices: return plan_slices(f, o);
  case CommittedFrame::Isovalues: return plan_isosurface(f, o);
  case CommittedFrame::Projection: return plan_projection(f, o);
  case CommittedFrame::March: break;
  }
  if (f.preintegrated && f.shading == 0) return plan_preintegrated(f, o); // under GRADIENT or FULL shading the mode is kept and not drawn
  if (gradient_opacity_active(f.gradient_opacity ? kGradientOpacityRamp : kGradientOpacityOff, true, f.shading, false))
    return plan_gradient_opacity(f, o); // under FULL shading, and behind an active pre-integration, the mode is kept and not drawn
  if (depth_output_active(f.depth_output, true, f.shading, false, false)) // (pre-integration and gradient opacity returned above)
    return plan_depth_output(f, o); // under FULL shading the setting is kept and not drawn; a committed depth image is applied by this kernel (f.max_depth)
  if (max_depth_active(f.max_depth, true, f.shading, false, false, true)) // (pre-integration and gradient opacity returned above; the host compared the sizes)
    return plan_max_depth(f, o); // under FULL shading the image is kept and not drawn
  LaunchPlan pl;
  pl.shading = f.shading == 0 || f.shading == 1 ? f.shading : 2;
  pl.orthographic = f.orthographic;
  const bool clip = f.clip_on || f.orthographic; // an orthographic frame is a clipped frame: with the unit box where no clip box is committed
  // the shadow cache: full shading without the shadow march is the gradient-shaded kernel plus one tap - everything below follows from SHADE 1 (no clipped
  // shade kernel: the clip is baked into the lattice; no shade order: there are no light beams to sort by) but the material flag, which the cached variants ride on
  pl.cached = pl.shading == 2 && f.shadow_cache;
  if (pl.cached) pl.shading = 1;
  const int sh = pl.shading;
  const Addressing a = plan_addressing(f, o);
  const size_t tf = tf_lds_bytes(f.n_color, f.n_alpha);
  if (a.error || tf == 0) { pl.error = true; return pl; }
  const int am = pl.am = a.am;
  pl.skip = f.skipping;
  pl.pooled = sh != 0 && f.pool;
  const size_t tables = align16(axis_table_bytes(f.nx, f.ny, f.nz, am));
  const size_t queues = (size_t)kWaves * request_queue_entries(sh, pl.pooled) * kShadeReqBytes;
  if (!pl.pooled) {
    pl.march_lds_bytes = std::max<size_t>(tf + tables + queues, (size_t)kWaves * kCounterWords * 4); // the counter reduction reuses it
    // a clipped frame takes the ordinary march (the same frame, and no further set of kernels), and where that shades, its material variant
    if (f.f32_general && sh == 0 && !f.skipping && am <= 1 && f.lds_staging && !f.sparse && !clip) {
      pl.march.lds_staged = true; // [.. tables, TF ..][bricks][region descriptor][corner rays 4 x float3][t range]
      pl.lds_brick_offset = (unsigned int)align16(pl.march_lds_bytes);
      pl.march_lds_bytes = pl.lds_brick_offset + (size_t)kLdsBrickCap * 128 + kLdsRegionBytes + 12 * 4 + 2 * 4 + 16;
    }
    else {
      pl.march.clipped = clip;
      pl.march.material = sh != 0 && (clip || !f.reference_material || pl.cached);
    }
    return pl;
  }
  pl.march_lds_bytes = queues + tables + (size_t)f.n_alpha * 4 + 64;
  pl.march.clipped = clip;
  pl.march.deep = !f.skipping && (am <= 1 || am == 4) && !clip && deep_rounds_pay(f, o); // a small image shard: the longest ray's chain of rounds is the floor
  pl.shade.clipped = sh == 2 && clip; // shadow rays are clipped too; without them the shade kernel never tests the box
  pl.shade.material = pl.shade.clipped || !f.reference_material || pl.cached || f.orthographic; // (orthographic: the view vector's twin rides on it)
  pl.shade_order = sh == 2 && f.shade_order; // no shadow rays: creation order (its tickets' batches, profiles/r02_notes.md section 11)
  pl.shade_lds_bytes = std::max<size_t>(tf + tables, 64);
  const int blocks = o.shade_blocks > 0 ? o.shade_blocks : f.shade_blocks;
  pl.shade_grid_blocks = blocks > 0 ? std::min(blocks, kShadeBlocks) : kShadeBlocks;
  return pl;
}

// the kind of frame a plan draws - the kernel family in the march's place - derived from the plan's own members: nothing is stored, nothing can disagree.  THE
// one reading of those members: plan_variants_exist, plan_kernels and the launchers of the known-answer queries (ovr_hip_kernels.hip) and what host/frame.cpp does
// behind a frame all switch over it.  (An error plan reads as the march: plan_variants_exist and plan_kernels ask `error` first)
inline FrameKind frame_kind(const LaunchPlan& pl)
{
  if (pl.preintegrated.on) return FrameKind::PreintegratedMarch;
  if (pl.gradient_opacity.on) return FrameKind::GradientOpacityMarch;
  if (pl.max_depth.on) return FrameKind::DepthLimitedMarch;
  if (pl.depth_output.on) return FrameKind::DepthOutputMarch;
  if (pl.slices.on) return pl.slices.context ? FrameKind::SliceContext : pl.slices.walks ? FrameKind::SliceWalk : FrameKind::SlicePlane;
  if (pl.isosurface.on)
    return pl.isosurface.context ? FrameKind::IsosurfaceContext : pl.ambient_occlusion ? FrameKind::IsosurfaceAo
           : pl.isosurface.translucent ? FrameKind::IsosurfaceLayers : FrameKind::Isosurface;
  return pl.project.mode != 0 ? FrameKind::Projection : FrameKind::March;
}

// the plan's variants exist - what frame_kernels / project_kernels_of / isosurface_kernels_of ... (the device headers: tables these predicates fill) then look up (f32_general decides the LDS-staged march alone)
inline bool plan_variants_exist(const LaunchPlan& pl, bool f32_general)
{
  if (pl.error) return false;
  switch (frame_kind(pl)) {
  case FrameKind::SlicePlane: case FrameKind::SliceWalk: case FrameKind::SliceContext:
    return slice_variant_exists(pl.slices.walks, pl.am, pl.slices.skip, pl.slices.clipped, pl.orthographic, pl.slices.context);
  case FrameKind::Isosurface: case FrameKind::IsosurfaceLayers: case FrameKind::IsosurfaceAo: case FrameKind::IsosurfaceContext:
    return isosurface_variant_exists(pl.shading, pl.am, pl.isosurface.skip, pl.isosurface.clipped, pl.orthographic, pl.isosurface.translucent, pl.ambient_occlusion, pl.isosurface.context);
  case FrameKind::Projection: return project_variant_exists(pl.project.mode, pl.am, pl.project.skip, pl.project.clipped, pl.orthographic);
  case FrameKind::PreintegratedMarch: return preintegrated_variant_exists(pl.am, pl.skip, pl.preintegrated.clipped, pl.orthographic);
  case FrameKind::GradientOpacityMarch: return gradient_opacity_variant_exists(pl.gradient_opacity.shade ? 1 : 0, pl.am, pl.skip, pl.gradient_opacity.clipped, pl.orthographic);
  case FrameKind::DepthLimitedMarch: return max_depth_variant_exists(pl.max_depth.shade ? 1 : 0, pl.am, pl.skip, pl.max_depth.clipped, pl.orthographic);
  case FrameKind::DepthOutputMarch: return depth_output_variant_exists(pl.depth_output.shade ? 1 : 0, pl.am, pl.skip, pl.depth_output.clipped, pl.orthographic);
  case FrameKind::March: break;
  }
  return march_variant_exists(pl.shading, pl.am, pl.pooled, pl.skip, pl.march.lds_staged, pl.march.deep, pl.march.material, pl.march.clipped, f32_general,
                              pl.cached && !pl.pooled, pl.orthographic) &&
         (!pl.pooled || shade_variant_exists(pl.shading, pl.am, pl.skip, pl.shade.material, pl.shade.clipped, pl.cached, pl.orthographic));
}
static_assert(!march_variant_exists(0, 0, false, false, false, false, false, false, true, false, true) && march_variant_exists(0, 0, false, false, false, false, false, true, true, false, true)
                && !march_variant_exists(0, 0, false, false, true, false, false, true, true, false, true) && !march_variant_exists(1, 0, true, false, false, true, false, true, false, false, true),
              "the orthographic march: on the clipped variants alone, never LDS-staged, never deep");
static_assert(shade_variant_exists(1, 0, false, true, false, false, true) && shade_variant_exists(2, 0, false, true, true, false, true) && !shade_variant_exists(2, 0, false, true, false, false, true)
                && !shade_variant_exists(1, 0, false, false, false, false, true) && shade_variant_exists(1, 0, false, true, false, true, true),
              "the orthographic shade kernel: the material variant - clipped where it marches shadow rays");
static_assert(project_variant_exists(kProjectMaximum, 0, true, true, true) && !project_variant_exists(kProjectMaximum, 0, true, false, true)
                && isosurface_variant_exists(2, 0, true, true, true) && !isosurface_variant_exists(2, 0, true, false, true),
              "the orthographic projection and isosurface kernels: on the clipped variants alone");
static_assert(isosurface_variant_exists(2, 0, true, true, false, true) && isosurface_variant_exists(0, 4, false, true, true, true) && !isosurface_variant_exists(2, 0, true, false, false, true),
              "the translucent isosurface kernels: on the clipped variants alone, for both cameras");
static_assert(isosurface_variant_exists(1, 0, false, true, false, true, true) && isosurface_variant_exists(2, 4, true, true, true, true, true) && !isosurface_variant_exists(0, 0, false, true, false, true, true)
                && !isosurface_variant_exists(2, 0, false, true, false, false, true) && !isosurface_variant_exists(2, 0, false, false, false, true, true),
              "the ambient-occlusion isosurface kernels: twins of the translucent ones, under a shading mode with an ambient term");
static_assert(slice_variant_exists(false, 0, false, true, true) && slice_variant_exists(true, 4, true, true, true) && !slice_variant_exists(true, 0, true, false, true)
                && !slice_variant_exists(false, 0, false, false, true) && !slice_variant_exists(false, 0, true, true),
              "the slice kernels: orthographic on the clipped variants alone; the plane kernel has no skipping twin");
static_assert(slice_variant_exists(false, 0, false, true, false, true) && slice_variant_exists(true, 4, false, true, true, true) && !slice_variant_exists(true, 0, false, false, false, true)
                && !slice_variant_exists(true, 0, true, true, false, true),
              "the slice context kernel: on the clipped variants alone, for both cameras, without a skipping twin");
static_assert(isosurface_variant_exists(0, 0, false, true, false, true, false, true) && isosurface_variant_exists(2, 4, false, true, true, true, false, true)
                && !isosurface_variant_exists(2, 0, false, false, false, true, false, true) && !isosurface_variant_exists(2, 0, true, true, false, true, false, true)
                && !isosurface_variant_exists(2, 0, false, true, false, true, true, true) && !isosurface_variant_exists(1, 0, false, true, false, false, false, true),
              "the isosurface context kernel: a translucent kernel on the clipped variants alone, for both cameras, without a skipping or an AO twin");
static_assert(preintegrated_variant_exists(0, false, true) && preintegrated_variant_exists(4, false, true, true) && !preintegrated_variant_exists(0, false, false)
                && !preintegrated_variant_exists(0, true, true) && !preintegrated_variant_exists(5, false, true),
              "the pre-integrated kernel: on the clipped variants alone, for both cameras, without a skipping twin");
static_assert(gradient_opacity_variant_exists(0, 0, false, true) && gradient_opacity_variant_exists(1, 4, false, true, true) && !gradient_opacity_variant_exists(2, 0, false, true)
                && !gradient_opacity_variant_exists(0, 0, false, false) && !gradient_opacity_variant_exists(1, 0, true, true) && !gradient_opacity_variant_exists(0, 5, false, true),
              "the gradient-opacity kernel: shading NONE and GRADIENT, on the clipped variants alone, for both cameras, without a skipping twin");
static_assert(max_depth_variant_exists(0, 0, false, true) && max_depth_variant_exists(1, 4, false, true, true) && !max_depth_variant_exists(2, 0, false, true)
                && !max_depth_variant_exists(0, 0, false, false) && !max_depth_variant_exists(1, 0, true, true) && !max_depth_variant_exists(0, 5, false, true),
              "the depth-limited kernel: shading NONE and GRADIENT, on the clipped variants alone, for both cameras, without a skipping twin");
static_assert(depth_output_variant_exists(0, 0, false, true) && depth_output_variant_exists(1, 4, false, true, true) && !depth_output_variant_exists(2, 0, false, true)
                && !depth_output_variant_exists(0, 0, false, false) && !depth_output_variant_exists(1, 0, true, true) && !depth_output_variant_exists(0, 5, false, true),
              "the depth-output kernel: the depth-limited kernel's variants");
static_assert((int)FrameKind::DepthOutputMarch == (int)FrameKind::DepthLimitedMarch + 1, "new frame kinds are appended: the ids of the others stay");
static_assert(kPreintegrationLdsBudget % 16 == 0 && 3 * kPreintegrationLdsBudget <= 160 * 1024 && 4 * kPreintegrationLdsBudget > 160 * 1024, "three workgroups per CU");

} // namespace ovrhip
