// device_hip.cpp - the reference-side binding of the MI355X backend: `DeviceHIP : ovr::MainRenderer`.
//
// Compiled AGAINST THE REFERENCE'S OWN HEADERS (-I$OVR_ROOT ...; nothing of the reference is copied here) into
// libdevice_hip.so, which exports the one symbol the reference's factory looks up for `--device hip`:
//     extern "C" ovr::MainRenderer* ovr_create_renderer__hip();
// (create_renderer -> LibraryRepository::add("device_hip") -> dlopen("libdevice_hip.so") -> objectFactory<MainRenderer>,
//  reference ovr/renderer.cpp:55-58, ovr/common/dylink/ObjectFactory.h:35-85).  The reference's apps (renderbatch,
// renderapp) run unmodified.  Everything below only forwards to the C ABI of include/ovr_hip.h - it plays the role
// ovr/devices/optix7/device.cpp + device_impl.cpp play for the OptiX device.
#include <ovr/renderer.h>

#include "../include/ovr_hip.h"
#include "isovalues_env.hpp"
#include "orthographic_env.hpp"
#include "slices_env.hpp"
#include "slice_context_env.hpp"
#include "iso_context_env.hpp"
#include "../open-volume-renderer_amd/csrc/host/preintegration_host.hpp" // (HIP-free: parse_preintegration)
#include "../open-volume-renderer_amd/csrc/host/gradient_opacity_host.hpp" // (HIP-free: parse_gradient_opacity)
#include "../open-volume-renderer_amd/csrc/host/max_depth_host.hpp" // (HIP-free: max_depth_read_file)
#include "../open-volume-renderer_amd/csrc/host/depth_output_host.hpp" // (HIP-free: parse_depth_output, depth_output_write_file)

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

void check(int code)
{
  if (code != 0) throw std::runtime_error(ovr_hip_last_error()); // the reference reports device errors as std::runtime_error
}

// The reference links its noise tile into the CUDA device's translation unit (ovr/CMakeLists.txt:67-72, blue_noise.h:74-79),
// out of a plugin's reach.  The same files ship in the reference's data/noise/: the tile is read from $OVR_HIP_NOISE_TILE or,
// failing that, from the names the reference's own (commented-out) file loader used, next to the executable.
// Layout [y][x][t] float32, t = 64 (blue_noise.h:95-99); xy follows from the file size.
bool load_noise_tile(ovr_hip_renderer* h)
{
  std::vector<std::string> candidates;
  if (const char* e = std::getenv("OVR_HIP_NOISE_TILE")) candidates.push_back(e);
  for (const char* name : { "stbn_128x128x64.bin", "blue_64x64x64.bin" }) { // STBN is the reference's default (generate_mask.h:9)
    candidates.push_back(std::string("./") + name);
    candidates.push_back(std::string("./data/noise/") + name);
    if (const char* root = std::getenv("OVR_ROOT")) candidates.push_back(std::string(root) + "/data/noise/" + name);
  }
  for (const std::string& path : candidates) {
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) continue;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    const long xy = bytes > 0 ? std::lround(std::sqrt((double)bytes / (64.0 * sizeof(float)))) : 0;
    std::vector<float> tile;
    bool ok = xy > 0 && (long)(xy * xy * 64 * sizeof(float)) == bytes;
    if (ok) {
      tile.resize((size_t)xy * xy * 64);
      ok = std::fread(tile.data(), 1, (size_t)bytes, f) == (size_t)bytes;
    }
    std::fclose(f);
    if (!ok) throw std::runtime_error("[hip] " + path + " is not an xy*xy*64 float32 noise tile");
    check(ovr_hip_set_noise_tile(h, tile.data(), (int32_t)xy));
    return true;
  }
  return false;
}

class DeviceHIP : public ovr::MainRenderer {
public:
  DeviceHIP() = default;
  ~DeviceHIP() override
  {
    if (h && convergence_mode != OVR_HIP_CONVERGENCE_OFF && !(std::getenv("OVR_HIP_QUIET") && std::getenv("OVR_HIP_QUIET")[0] != '0')) {
      ovr_hip_convergence c;
      if (ovr_hip_get_convergence(h, &c) == 0)
        std::fprintf(stderr, "[hip] convergence: error %g after %d frames, %d of %d blocks retired\n", (double)c.error, c.frames, c.retired_blocks, c.blocks);
    }
    // OVR_HIP_DEPTH_OUTPUT_FILE: the last mapped depth frame's resolved threshold depth (see mapframe)
    if (const char* path = std::getenv("OVR_HIP_DEPTH_OUTPUT_FILE")) {
      const bool quiet = std::getenv("OVR_HIP_QUIET") && std::getenv("OVR_HIP_QUIET")[0] != '0';
      if (depth_layer.empty()) std::fprintf(stderr, "[hip] OVR_HIP_DEPTH_OUTPUT_FILE: the last mapped frame was no depth frame (OVR_HIP_DEPTH_OUTPUT, OVR_HIP_MAP_GRAD): nothing is written\n");
      else if (!ovrhip::depth_output_write_file(path, depth_layer.data(), depth_w, depth_h)) std::fprintf(stderr, "[hip] OVR_HIP_DEPTH_OUTPUT_FILE: %s could not be written\n", path);
      else if (!quiet) std::fprintf(stderr, "[hip] depth output: %d x %d threshold depths written to %s\n", depth_w, depth_h, path);
    }
    ovr_hip_destroy(h);
  }
  DeviceHIP(const DeviceHIP&) = delete;
  DeviceHIP& operator=(const DeviceHIP&) = delete;

  // DeviceOptix7::init -> Impl::init -> buildScene (optix7/device.cpp:16-20, device_impl.cpp:283-302)
  void init(int argc, const char** argv) override
  {
    if (h) throw std::runtime_error("[hip] device already initialized!");
    // One GPU (`--hip-device N`, default 0: the reference hard-codes device 0, device_impl.cpp:371-372) or several behind this one
    // MainRenderer: `--hip-devices 0,1,2,...` or OVR_HIP_DEVICES=0,1,2,... (the unmodified apps pass no such flag: the environment
    // variable is their switch).  The group shards the image plane into tiles over the listed devices and gathers them on the first
    // (ovr_hip_create_group); everything below is the same for both.
    std::string list = std::getenv("OVR_HIP_DEVICES") ? std::getenv("OVR_HIP_DEVICES") : "";
    int device_id = 0;
    bool no_skip_flag = false;
    for (int i = 1; i < argc; ++i) {
      if (std::string(argv[i]) == "--hip-no-skip") no_skip_flag = true; // = OVR_HIP_SKIP_EMPTY=0 (a host that forwards its arguments; the reference's
      if (i + 1 >= argc) continue;                                      // own apps reject flags they do not know - args::ParseError - and use the variable)
      if (std::string(argv[i]) == "--hip-device") device_id = std::stoi(argv[i + 1]);
      if (std::string(argv[i]) == "--hip-devices") list = argv[i + 1];
    }
    std::vector<int32_t> devices;
    for (size_t at = 0; at < list.size();) {
      const size_t comma = list.find(',', at);
      const std::string tok = list.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
      if (!tok.empty()) devices.push_back((int32_t)std::stoi(tok));
      if (comma == std::string::npos) break;
      at = comma + 1;
    }
    if (devices.empty()) check(ovr_hip_create(&h, device_id));
    else check(ovr_hip_create_group(&h, devices.data(), (int32_t)devices.size()));
    const auto& v = ovr::parse_single_volume_scene(current_scene, ovr::scene::Volume::STRUCTURED_REGULAR_VOLUME).structured_regular;
    const int32_t dims[3] = { v.data->dims.x, v.data->dims.y, v.data->dims.z };
    const float origin[3] = { v.grid_origin.x, v.grid_origin.y, v.grid_origin.z };
    const float spacing[3] = { v.grid_spacing.x, v.grid_spacing.y, v.grid_spacing.z };
    check(ovr_hip_set_volume(h, v.data->data(), OVR_HIP_MEM_HOST, (int)v.data->type, dims, origin, spacing));
    check(ovr_hip_set_volume_sampling_rate(h, current_scene.volume_sampling_rate)); // device_impl.cpp:298
    check(ovr_hip_set_shading(h, OVR_HIP_SHADE_FULL));                             // what the reference's marcher does
    // The reference builds its macrocell grids for every volume / transfer function (accel/sp_singlemc.cu) but only its path
    // tracer walks them; here the ray marcher skips empty space with them - the frames are bit-identical, so the drop-in
    // device has it on (OVR_HIP_SKIP_EMPTY=0 switches it off, e.g. to count every sample like the reference)
    // (any fps quoted through this device must say which: with skipping the march fetches a fraction of the reference's samples - C3: 889 vs 373 fps)
    const char* skip = std::getenv("OVR_HIP_SKIP_EMPTY");
    const bool skipping = !(no_skip_flag || (skip && skip[0] == '0'));
    check(ovr_hip_set_empty_space_skipping(h, skipping ? 1 : 0));
    if (!(std::getenv("OVR_HIP_QUIET") && std::getenv("OVR_HIP_QUIET")[0] != '0'))
      std::fprintf(stderr, "[hip] empty-space skipping %s\n", skipping ? "ON (bit-identical frames, fewer samples fetched than the reference's marcher; OVR_HIP_SKIP_EMPTY=0 / --hip-no-skip: the reference's exact work)"
                                                                      : "OFF (every sample fetched, like the reference's marcher)");
    // nothing behind this interface reads per-phase device times: no events between the frame's kernels (OVR_HIP_PHASE_TIMING=1 keeps them)
    const char* phases = std::getenv("OVR_HIP_PHASE_TIMING");
    check(ovr_hip_set_phase_timing(h, (phases && phases[0] == '1') ? 1 : 0));
    // MainRenderer::variance (ovr/renderer.h:124-127,287) - what renderapp shows in its title bar and renderbatch's progressive loop stops on - is the frame
    // error of the convergence estimate when OVR_HIP_CONVERGENCE=1 (estimate only: same frames) or =2 (blocks whose error is <= OVR_HIP_CONVERGENCE_THRESHOLD,
    // default 0, are retired: no longer marched).  Unset: 0, like the reference's OptiX device (device_impl.cpp:266)
    if (const char* cv = std::getenv("OVR_HIP_CONVERGENCE")) {
      convergence_mode = std::atoi(cv);
      const char* th = std::getenv("OVR_HIP_CONVERGENCE_THRESHOLD");
      check(ovr_hip_set_convergence(h, convergence_mode, th ? (float)std::atof(th) : 0.f));
    }
    // OVR_HIP_RECONSTRUCT=1: frames rendered with sparse sampling on ("Sparse Sampling" in renderapp) are completed by the pull-push reconstruction
    //  before they are mapped; off by default, like the reference, whose sparse frames are mostly holes
    {
      const char* rc = std::getenv("OVR_HIP_RECONSTRUCT");
      const int mode = (rc && rc[0] == '1') ? OVR_HIP_RECONSTRUCT_FILL : OVR_HIP_RECONSTRUCT_OFF;
      if (mode != OVR_HIP_RECONSTRUCT_OFF) check(ovr_hip_set_reconstruction(h, mode));
      if (rc && !(std::getenv("OVR_HIP_QUIET") && std::getenv("OVR_HIP_QUIET")[0] != '0'))
        std::fprintf(stderr, "[hip] reconstruction of sparse-sampled frames: %s\n", mode == OVR_HIP_RECONSTRUCT_FILL ? "on (pull-push fill)" : "off");
    }
    // The interface's lighting controls (set_light_phi / _theta / _intensity, set_mat_*: renderapp's sliders) are forwarded by commit() below.  The batch app
    // has no sliders: OVR_HIP_LIGHT=phi,theta[,intensity] (degrees) and OVR_HIP_MATERIAL=ambient,diffuse,specular,shininess set them once.  Unset: nothing
    // is called, the frames are the reference's literal light and shade expression
    {
      const bool quiet = std::getenv("OVR_HIP_QUIET") && std::getenv("OVR_HIP_QUIET")[0] != '0';
      if (const char* lv = std::getenv("OVR_HIP_LIGHT")) {
        float a[3] = { 0.f, 0.f, intensity };
        const int n = std::sscanf(lv, "%f,%f,%f", &a[0], &a[1], &a[2]);
        if (n < 2) throw std::runtime_error("[hip] OVR_HIP_LIGHT expects phi,theta[,intensity] in degrees");
        phi = a[0]; theta = a[1]; intensity = a[2];
        angles_set = true;
        push_light();
        if (!quiet) std::fprintf(stderr, "[hip] light: phi %g, theta %g degrees, intensity %g\n", (double)phi, (double)theta, (double)intensity);
      }
      if (const char* mv = std::getenv("OVR_HIP_MATERIAL")) {
        if (std::sscanf(mv, "%f,%f,%f,%f", &material[0], &material[1], &material[2], &material[3]) != 4)
          throw std::runtime_error("[hip] OVR_HIP_MATERIAL expects ambient,diffuse,specular,shininess");
        check(ovr_hip_set_material(h, material[0], material[1], material[2], material[3]));
        if (!quiet) std::fprintf(stderr, "[hip] material: ambient %g, diffuse %g, specular %g, shininess %g\n", (double)material[0], (double)material[1], (double)material[2], (double)material[3]);
      }
      // The clip box (ovr_hip_set_clip_box): the scene file's view.volume.clippingBox never reaches a device - the reference's loader discards it - so
      // OVR_HIP_CLIP_BOX=x0,y0,z0,x1,y1,z1 (world units: the space of the volume's grid_origin / grid_spacing; inf / -inf leave a side open) is the
      // batch app's only switch.  Unset: nothing is called
      if (const char* cv = std::getenv("OVR_HIP_CLIP_BOX")) {
        float lo[3], hi[3];
        if (std::sscanf(cv, "%f,%f,%f,%f,%f,%f", &lo[0], &lo[1], &lo[2], &hi[0], &hi[1], &hi[2]) != 6)
          throw std::runtime_error("[hip] OVR_HIP_CLIP_BOX expects x0,y0,z0,x1,y1,z1 in world units");
        check(ovr_hip_set_clip_box(h, lo, hi));
        if (!quiet) std::fprintf(stderr, "[hip] clip box (%g, %g, %g) .. (%g, %g, %g)\n", (double)lo[0], (double)lo[1], (double)lo[2], (double)hi[0], (double)hi[1], (double)hi[2]);
      }
      // The shadow cache (ovr_hip_set_shadow_cache): OVR_HIP_SHADOW_CACHE=<cell> takes the shadow term of the full shading from a lattice of one node per
      // <cell> voxels (0 = the library's default cell).  Unset: nothing is called, the frames march their shadow rays
      if (const char* sv = std::getenv("OVR_HIP_SHADOW_CACHE")) {
        int cell = 0;
        if (std::sscanf(sv, "%d", &cell) != 1 || cell < 0) throw std::runtime_error("[hip] OVR_HIP_SHADOW_CACHE expects the cell size in voxels (0 = the default)");
        check(ovr_hip_set_shadow_cache(h, OVR_HIP_SHADOWS_CACHED, cell));
        if (!quiet) std::fprintf(stderr, "[hip] shadow cache: one node per %d voxels%s\n", cell > 0 ? cell : 4, cell > 0 ? "" : " (the default)");
      }
      // Projections (ovr_hip_set_projection): OVR_HIP_PROJECTION=max|min|mean renders the maximum, minimum or mean intensity projection in the march's
      // place, classified by the scene's transfer function.  Unset: nothing is called, the frames are the march's
      if (const char* pv = std::getenv("OVR_HIP_PROJECTION")) {
        const std::string p(pv);
        const int mode = p == "max" ? OVR_HIP_PROJECT_MAXIMUM : p == "min" ? OVR_HIP_PROJECT_MINIMUM : p == "mean" ? OVR_HIP_PROJECT_MEAN : -1;
        if (mode < 0) throw std::runtime_error("[hip] OVR_HIP_PROJECTION expects max, min or mean");
        check(ovr_hip_set_projection(h, mode));
        if (!quiet) std::fprintf(stderr, "[hip] projection: %s intensity\n", p == "max" ? "maximum" : p == "min" ? "minimum" : "mean");
      }
      // Isosurfaces (ovr_hip_set_isosurfaces): OVR_HIP_ISOVALUES=0.4,0.7 draws the level sets of up to four isovalues (the samples' units: 8-bit volumes
      // normalised) in the march's place, coloured by the scene's transfer function, shaded by the scene's shading mode.  Unset: nothing is called
      if (const char* iv = std::getenv("OVR_HIP_ISOVALUES")) {
        float v[OVR_HIP_MAX_ISOVALUES + 1];
        const int n = ovrhip_plugin::parse_isovalues(iv, v, OVR_HIP_MAX_ISOVALUES); // (the whole string: trailing text is an error, not a shorter list)
        if (n < 1) throw std::runtime_error("[hip] OVR_HIP_ISOVALUES expects one to four isovalues separated by commas");
        // OVR_HIP_ISO_OPACITIES=0.3,1 beside it (ovr_hip_set_isosurface_layers): one opacity in (0, 1] per isovalue, in the isovalues' order - translucent level
        // sets, every crossing composited.  Unset: the opaque call, nothing changes
        float a[OVR_HIP_MAX_ISOVALUES + 1];
        const char* ov = std::getenv("OVR_HIP_ISO_OPACITIES");
        if (ov && ovrhip_plugin::parse_iso_opacities(ov, a, n) != n)
          throw std::runtime_error("[hip] OVR_HIP_ISO_OPACITIES expects one opacity in (0, 1] per isovalue of OVR_HIP_ISOVALUES, separated by commas");
        check(ov ? ovr_hip_set_isosurface_layers(h, v, a, n) : ovr_hip_set_isosurfaces(h, v, n));
        if (!quiet) {
          std::fprintf(stderr, "[hip] isosurfaces at");
          for (int k = 0; k < n; ++k) std::fprintf(stderr, "%s %g", k ? "," : "", (double)v[k]);
          if (ov) {
            std::fprintf(stderr, " with opacities");
            for (int k = 0; k < n; ++k) std::fprintf(stderr, "%s %g", k ? "," : "", (double)a[k]);
          }
          std::fprintf(stderr, "\n");
        }
      }
      // Isosurface context (ovr_hip_set_isosurface_context): OVR_HIP_ISO_CONTEXT=<scale in [0, 1]> beside OVR_HIP_ISOVALUES marches the unshaded volume around
      // the level sets in the same walk, every corrected opacity of the volume multiplied by the scale.  Unset: OFF, nothing is called
      if (const char* cv = std::getenv("OVR_HIP_ISO_CONTEXT")) {
        float scale = 1.f;
        if (!ovrhip_plugin::parse_iso_context(cv, &scale)) throw std::runtime_error("[hip] OVR_HIP_ISO_CONTEXT expects one opacity scale in [0, 1]");
        check(ovr_hip_set_isosurface_context(h, OVR_HIP_ISO_CONTEXT_VOLUME, scale));
        if (!quiet) std::fprintf(stderr, "[hip] isosurface context: the volume around the level sets, opacity scale %g\n", (double)scale);
      }
      // Ambient occlusion of the isosurface frames (ovr_hip_set_ambient_occlusion): OVR_HIP_AO_SAMPLES=8 casts that many occlusion walks per event,
      // OVR_HIP_AO_DISTANCE=12 cuts them at that many world units (unset: the whole box).  Unset: nothing is called (the scene's own ao_samples is not read)
      if (const char* as = std::getenv("OVR_HIP_AO_SAMPLES")) {
        int k = 0;
        float dist = 0.f;
        const char* ad = std::getenv("OVR_HIP_AO_DISTANCE");
        if (ovrhip_plugin::parse_ao(as, ad, &k, &dist) != 0)
          throw std::runtime_error("[hip] OVR_HIP_AO_SAMPLES expects an integer in 0 ... 16, OVR_HIP_AO_DISTANCE a distance > 0 or inf");
        check(ovr_hip_set_ambient_occlusion(h, k, dist));
        if (!quiet) std::fprintf(stderr, "[hip] ambient occlusion: %d samples within %g\n", k, (double)dist);
      }
      // Slices (ovr_hip_set_slices): OVR_HIP_SLICES="px,py,pz,nx,ny,nz[,thickness[,max|min|mean]];..." draws up to four cut planes (thickness 0, the default)
      // or thick slabs (world units along the normal; inf: the whole box) in the march's place, coloured by the scene's transfer function.  Unset: nothing is called
      if (const char* sv = std::getenv("OVR_HIP_SLICES")) {
        ovrhip_plugin::SliceEnv e[OVR_HIP_MAX_SLICES];
        const int n = ovrhip_plugin::parse_slices(sv, e, OVR_HIP_MAX_SLICES); // (the whole string: trailing text is an error, not a shorter list)
        if (n < 1) throw std::runtime_error("[hip] OVR_HIP_SLICES expects one to four slices px,py,pz,nx,ny,nz[,thickness[,max|min|mean]] separated by semicolons");
        ovr_hip_slice sl[OVR_HIP_MAX_SLICES];
        for (int k = 0; k < n; ++k) {
          for (int a = 0; a < 3; ++a) { sl[k].point[a] = e[k].point[a]; sl[k].normal[a] = e[k].normal[a]; }
          sl[k].thickness = e[k].thickness;
          sl[k].mode = e[k].mode;
        }
        check(ovr_hip_set_slices(h, sl, n));
        if (!quiet)
          for (int k = 0; k < n; ++k)
            std::fprintf(stderr, "[hip] slice %d: through (%g, %g, %g), normal (%g, %g, %g), %s%s\n", k, (double)e[k].point[0], (double)e[k].point[1], (double)e[k].point[2],
                         (double)e[k].normal[0], (double)e[k].normal[1], (double)e[k].normal[2],
                         e[k].thickness > 0.f ? (e[k].mode == 1 ? "a maximum slab" : e[k].mode == 2 ? "a minimum slab" : "a mean slab") : "a plane",
                         e[k].thickness > 0.f ? (std::string(" of thickness ") + std::to_string(e[k].thickness)).c_str() : "");
      }
      // Slice context (ovr_hip_set_slice_context): OVR_HIP_SLICE_CONTEXT=<scale in [0, 1]> beside OVR_HIP_SLICES marches the unshaded volume in front of the
      // slices, every corrected opacity multiplied by the scale.  Unset: OFF, nothing is called
      if (const char* cv = std::getenv("OVR_HIP_SLICE_CONTEXT")) {
        float scale = 1.f;
        if (!ovrhip_plugin::parse_slice_context(cv, &scale)) throw std::runtime_error("[hip] OVR_HIP_SLICE_CONTEXT expects one opacity scale in [0, 1]");
        check(ovr_hip_set_slice_context(h, OVR_HIP_SLICE_CONTEXT_FRONT, scale));
        if (!quiet) std::fprintf(stderr, "[hip] slice context: the volume in front of the slices, opacity scale %g\n", (double)scale);
      }
      // Pre-integrated classification (ovr_hip_set_preintegration): OVR_HIP_PREINTEGRATION=1 classifies every segment of the unshaded march by the transfer
      // function's integral over the values it spans; 0: OFF.  Unset: nothing is called
      if (const char* pv = std::getenv("OVR_HIP_PREINTEGRATION")) {
        int mode = 0;
        if (!ovrhip::parse_preintegration(pv, &mode)) throw std::runtime_error("[hip] OVR_HIP_PREINTEGRATION expects 0 or 1");
        check(ovr_hip_set_preintegration(h, mode));
        if (!quiet && mode) std::fprintf(stderr, "[hip] pre-integrated classification: segments (drawn by unshaded march frames)\n");
      }
      // Gradient opacity (ovr_hip_set_gradient_opacity): OVR_HIP_GRADIENT_OPACITY=lo,hi weights every sample's table opacity by the ramp over the gradient's
      // magnitude, in transfer-function ranges per world unit length.  Unset: nothing is called
      if (const char* gv = std::getenv("OVR_HIP_GRADIENT_OPACITY")) {
        float lo = 0.f, hi = 1.f;
        if (!ovrhip::parse_gradient_opacity(gv, &lo, &hi)) throw std::runtime_error("[hip] OVR_HIP_GRADIENT_OPACITY expects lo,hi: two finite numbers with lo < hi");
        check(ovr_hip_set_gradient_opacity(h, OVR_HIP_GRADIENT_OPACITY_RAMP, lo, hi));
        if (!quiet) std::fprintf(stderr, "[hip] gradient opacity: ramp %g ... %g (drawn by march frames under shading NONE or GRADIENT)\n", (double)lo, (double)hi);
      }
      // The depth layer (ovr_hip_set_depth_output): OVR_HIP_DEPTH_OUTPUT=<threshold>, a number in (0, 0.9999] - the accumulated opacity at which a ray counts as
      // having reached its surface.  The gradient layer of a march frame under shading NONE or GRADIENT then carries (d, S, reached), depths in the march's t: the
      // unit OVR_HIP_MAX_DEPTH takes.  OVR_HIP_DEPTH_OUTPUT_FILE=<path>: when the renderer is destroyed the last mapped frame's resolved threshold depth is written
      // there as raw little-endian float32 in the frame's pixel order, +inf where not reached - exactly the file OVR_HIP_MAX_DEPTH reads.  Unset: nothing is called
      if (const char* zv = std::getenv("OVR_HIP_DEPTH_OUTPUT")) {
        float tau = 0.f;
        if (!ovrhip::parse_depth_output(zv, &tau))
          throw std::runtime_error("[hip] OVR_HIP_DEPTH_OUTPUT expects a threshold in (0, 0.9999]");
        check(ovr_hip_set_depth_output(h, OVR_HIP_DEPTH_OUTPUT_ON, tau));
        if (!quiet) std::fprintf(stderr, "[hip] depth output: threshold %g (drawn by march frames under shading NONE or GRADIENT; the gradient layer carries the depth)\n", (double)tau);
      }
    }
    commit();
  }

  void swap() override { check(ovr_hip_swap(h)); }

  // DeviceOptix7::Impl::commit (device_impl.cpp:113-197): forward every changed TransactionalValue
  void commit() override
  {
    if (params.fbsize.update()) {
      check(ovr_hip_set_fbsize(h, params.fbsize.ref().x, params.fbsize.ref().y));
      // The depth limit (ovr_hip_set_max_depth): OVR_HIP_MAX_DEPTH=<path> names a raw little-endian float32 file of width * height ray parameters in the frame's
      // pixel order (pixel (ix, iy) at ix + iy * width), read whenever the framebuffer size is set.  UNITS: the march's t - world length along the normalised ray
      // direction from the ray's origin: under the perspective camera the Euclidean distance from the camera position, not a planar z and not a z-buffer value;
      // under the orthographic camera the distance from the image plane through `from`.  +inf or NaN: no surface at that pixel.  Unset: nothing is called
      if (const char* dv = std::getenv("OVR_HIP_MAX_DEPTH")) {
        const int w = params.fbsize.ref().x, ht = params.fbsize.ref().y;
        std::vector<float> depth;
        if (!ovrhip::max_depth_read_file(dv, w, ht, &depth))
          throw std::runtime_error("[hip] OVR_HIP_MAX_DEPTH expects a raw little-endian float32 file of exactly width * height values (" + std::to_string(w) + " x " + std::to_string(ht) + ")");
        check(ovr_hip_set_max_depth(h, depth.data(), OVR_HIP_MEM_HOST, w, ht));
        const bool quiet = std::getenv("OVR_HIP_QUIET") && std::getenv("OVR_HIP_QUIET")[0] != '0';
        if (!quiet) std::fprintf(stderr, "[hip] depth limit: %d x %d ray parameters from %s (drawn by march frames under shading NONE or GRADIENT)\n", w, ht, dv);
      }
    }
    if (params.camera.update()) {
      const ovr::scene::Camera& c = params.camera.ref();
      const float from[3] = { c.from.x, c.from.y, c.from.z }, at[3] = { c.at.x, c.at.y, c.at.z }, up[3] = { c.up.x, c.up.y, c.up.z };
      // The orthographic camera (ovr_hip_set_camera_orthographic): the interface's Camera::type, which the OSPRay device honours and the OptiX device never
      // reads.  The batch app's scene loader never sets the type, so OVR_HIP_ORTHOGRAPHIC=<height>|auto forces it: the image's world height, or `auto` = the
      // parallel view with the perspective view's extent at the plane through `at`, 2 |from - at| tan(fovy / 2).  Unset: the type decides
      float height = 0.f;
      int ortho = c.type == ovr::scene::Camera::ORTHOGRAPHIC ? ovrhip_plugin::kOrthographicHeight : 0;
      if (ortho) height = c.orthographic.height;
      if (const char* ov = std::getenv("OVR_HIP_ORTHOGRAPHIC")) {
        ortho = ovrhip_plugin::parse_orthographic(ov, &height); // (the whole string: anything but a height > 0 or `auto` is an error)
        if (ortho == ovrhip_plugin::kOrthographicError) throw std::runtime_error("[hip] OVR_HIP_ORTHOGRAPHIC expects the image's world height (> 0) or auto");
        if (ortho == ovrhip_plugin::kOrthographicAuto) height = ovrhip_plugin::auto_orthographic_height(from, at, c.perspective.fovy);
        const bool quiet = std::getenv("OVR_HIP_QUIET") && std::getenv("OVR_HIP_QUIET")[0] != '0';
        if (!quiet && height != said_height) std::fprintf(stderr, "[hip] orthographic camera: image height %g%s\n", (double)height, ortho == ovrhip_plugin::kOrthographicAuto ? " (auto)" : "");
        said_height = height;
      }
      if (ortho) check(ovr_hip_set_camera_orthographic(h, from, at, up, height));
      else check(ovr_hip_set_camera(h, from, at, up, c.perspective.fovy));
    }
    if (params.tfn.update()) {
      const auto& t = params.tfn.ref();
      check(ovr_hip_set_transfer_function(h, t.tfn_colors.data(), (int32_t)(t.tfn_colors.size() / 3), t.tfn_alphas.data(),
                                          (int32_t)(t.tfn_alphas.size() / 2), t.tfn_value_range.x, t.tfn_value_range.y));
    }
    const bool focus = params.focus_center.update() | params.focus_scale.update() | params.base_noise.update();
    if (focus)
      check(ovr_hip_set_focus(h, params.focus_center.ref().x, params.focus_center.ref().y, params.focus_scale.ref(), params.base_noise.ref()));
    if (params.sample_per_pixel.update()) check(ovr_hip_set_sample_per_pixel(h, params.sample_per_pixel.ref()));
    if (params.path_tracing.update() && params.path_tracing.ref())
      throw std::runtime_error("[hip] path tracing is not part of the ray-marching backend");
    if (params.sparse_sampling.update()) {
      if (params.sparse_sampling.ref() && !have_noise) {
        if (!load_noise_tile(h))
          throw std::runtime_error("[hip] sparse sampling needs the reference's noise tile: set OVR_HIP_NOISE_TILE to data/noise/stbn_128x128x64.bin "
                                   "(or blue_64x64x64.bin), or run next to it");
        have_noise = true;
      }
      check(ovr_hip_set_sparse_sampling(h, params.sparse_sampling.ref()));
    }
    if (params.frame_accumulation.update()) check(ovr_hip_set_frame_accumulation(h, params.frame_accumulation.ref()));
    if (params.volume_sampling_rate.update()) check(ovr_hip_set_volume_sampling_rate(h, params.volume_sampling_rate.get()));
    // the seven lighting controls (ovr/renderer.h:210-248; the OptiX device never reads them).  A member that was never set keeps the backend's value:
    // the state below starts as the reference's literals, and until an angle arrives the direction stays the literal vector itself (NULL)
    bool light_changed = false, material_changed = false;
    if (params.phi.update()) { phi = params.phi.ref(); angles_set = light_changed = true; }
    if (params.theta.update()) { theta = params.theta.ref(); angles_set = light_changed = true; }
    if (params.intensity.update()) { intensity = params.intensity.ref(); light_changed = true; }
    if (params.ambient.update()) { material[0] = params.ambient.ref(); material_changed = true; }
    if (params.diffuse.update()) { material[1] = params.diffuse.ref(); material_changed = true; }
    if (params.specular.update()) { material[2] = params.specular.ref(); material_changed = true; }
    if (params.shininess.update()) { material[3] = params.shininess.ref(); material_changed = true; }
    if (light_changed) push_light();
    if (material_changed) check(ovr_hip_set_material(h, material[0], material[1], material[2], material[3]));
    check(ovr_hip_commit(h));
  }

  // DeviceOptix7::render (optix7/device.cpp:35-43): blocking; elapsed milliseconds are added to render_time
  void render() override
  {
    const auto start = std::chrono::high_resolution_clock::now();
    check(ovr_hip_render(h));
    const auto end = std::chrono::high_resolution_clock::now();
    render_time += std::chrono::duration_cast<std::chrono::milliseconds>(end - start).count();
    variance = 0.f; // device_impl.cpp:266
    if (convergence_mode != OVR_HIP_CONVERGENCE_OFF) {
      ovr_hip_convergence c;
      check(ovr_hip_get_convergence(h, &c));
      variance = c.error; // +inf until the second accumulated frame
    }
  }

  // Impl::mapframe (device_impl.cpp:271-281).  The reference hands out device pointers (DEVICE_CUDA), which only exist
  // in its CUDA build; an app built without OVR_BUILD_CUDA_DEVICES knows DEVICE_CPU only, so the frame is mapped to host
  // memory owned by the backend - what the caller's to_cpu() (cross_device_buffer.h:130-159) would do next anyway.
  // Only the rectangle the volume's box projects into crosses PCIe (ovr_hip_mapframe).  OVR_HIP_MAP_GRAD=0 leaves the gradient layer unset
  // like the reference's OSPRay device does (ospray/device_impl.cpp:814-818) - 43 % of a mapped frame's bytes, read only by renderapp's
  // "gradient" view.
  void mapframe(FrameBufferData* fb) override
  {
    static const bool want_grad = !(std::getenv("OVR_HIP_MAP_GRAD") && std::getenv("OVR_HIP_MAP_GRAD")[0] == '0');
    const float *rgba = nullptr, *grad = nullptr;
    size_t nb_rgba = 0, nb_grad = 0;
    check(ovr_hip_mapframe(h, OVR_HIP_MEM_HOST, &rgba, &nb_rgba, want_grad ? &grad : nullptr, want_grad ? &nb_grad : nullptr));
    fb->rgba->set_data((void*)rgba, nb_rgba, ovr::CrossDeviceBuffer::DEVICE_CPU);
    if (want_grad) fb->grad->set_data((void*)grad, nb_grad, ovr::CrossDeviceBuffer::DEVICE_CPU);
    // OVR_HIP_DEPTH_OUTPUT_FILE: keep the layer of the last mapped frame while it is a depth frame's (the destructor resolves and writes it)
    static const bool want_depth_file = std::getenv("OVR_HIP_DEPTH_OUTPUT_FILE") != nullptr;
    if (want_depth_file) {
      ovr_hip_depth_output z;
      const int w = params.fbsize.ref().x, ht = params.fbsize.ref().y;
      depth_layer.clear();
      if (want_grad && grad && ovr_hip_get_depth_output(h, &z) == 0 && z.active && w > 0 && ht > 0 && nb_grad == (size_t)w * (size_t)ht * 3 * sizeof(float)) {
        depth_layer.assign(grad, grad + (size_t)w * (size_t)ht * 3);
        depth_w = w; depth_h = ht;
      }
    }
  }

private:
  // degrees -> (sin phi cos theta, sin phi sin theta, cos phi), in double, rounded to float per component (include/ovr_hip.h: ovr_hip_set_light)
  void push_light()
  {
    if (!angles_set) { check(ovr_hip_set_light(h, nullptr, intensity)); return; }
    const double p = (double)phi * M_PI / 180.0, t = (double)theta * M_PI / 180.0;
    const float d[3] = { (float)(std::sin(p) * std::cos(t)), (float)(std::sin(p) * std::sin(t)), (float)std::cos(p) };
    check(ovr_hip_set_light(h, d, intensity));
  }

  // the literal light's own angles (used for the angle that was not set when the other one is): acos(z / |L|), atan2(y, x) of params.h:79
  float phi = 99.52095708f, theta = 112.35362395f, intensity = 1.f;
  float material[4] = { 0.5f, 0.5f, 0.f, 0.f };
  bool angles_set = false;
  ovr_hip_renderer* h = nullptr;
  bool have_noise = false;
  std::vector<float> depth_layer; // OVR_HIP_DEPTH_OUTPUT_FILE: the layer (3 floats per pixel) of the last mapped frame, empty while that was no depth frame
  int depth_w = 0, depth_h = 0;
  float said_height = 0.f; // OVR_HIP_ORTHOGRAPHIC: the height last reported on stderr (the camera is forwarded with every change; said once per value)

  int convergence_mode = OVR_HIP_CONVERGENCE_OFF;
};

} // namespace

// OVR_REGISTER_OBJECT(MainRenderer, renderer, DeviceHIP, hip) would expand to this (ObjectFactory.h:77-85)
extern "C" ovr::MainRenderer* ovr_create_renderer__hip() { return new DeviceHIP; }
