// ref_march_probe.cpp - runs the reference's ray marcher (ovr/devices/optix7/shaders_raymarching.cu + shaders_common.h), compiled
// for the HOST from its unmodified text, over one scene and writes the frame it renders.  TEST INFRASTRUCTURE ONLY.
// This file holds no reference source: it #includes the shader by path at build time (oracle/build_ref.sh), with the CUDA / OptiX
// names coming from oracle/cuda_host_shim/.  What it restates is the HOST side that fills the shader's parameters, each step with the
// place it restates; the shader itself - ray generation, TEA jitter, box intersection, both marches, shading, blending, accumulation -
// is the reference's own text.
//
//   ref_march_probe <scene file> <output file>
//
// scene file (little endian, written by tests/golden/make_ref_march.py):
//   int32 magic 'OVRM', value_type (ovr/scene.h numbering), dims[3]; float origin[3], spacing[3]; int32 n_colors, n_alphas;
//   float tfn_range[2], cam_from[3], cam_at[3], cam_up[3], fovy; int32 width, height, spp; float rate;
//   int32 frames, accumulate, n_sparse, filter_fraction_bits;
//   voxels (x fastest); n_colors * 3 floats; n_alphas * 2 floats (position, alpha); n_sparse * 2 int32 (x, y)
// output file: width * height * 4 floats rgba, width * height * 3 floats grad (the last frame), uint64 primary iterations, uint64
//   shadow iterations (summed over all frames), 12 floats: the launch parameters' camera (position, direction, horizontal, vertical)
#include "shaders_common.h"
namespace ovr { namespace optix7 { typedef random::RandomTEA RandomTEA; } } // accel/spatial_partition.h:18-20 does this under __NVCC__ only
#include "shaders_raymarching.cu"

#include "cuda_host_shim/ovr_shim.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

static_assert(sizeof(ovr::optix7::LaunchParams::DeviceCamera) == 12 * sizeof(float), "the camera is four packed vec3f");

namespace ovr { namespace optix7 {
extern "C" { LaunchParams optix_launch_params; } // shaders_common.h:46 declares it; OptiX would fill it from the launch's buffer
} }

using namespace ovr;
using namespace ovr::optix7;

namespace {

struct Header {
  int32_t magic, value_type, dims[3];
  float origin[3], spacing[3];
  int32_t n_colors, n_alphas;
  float tfn_range[2], cam_from[3], cam_at[3], cam_up[3], fovy;
  int32_t width, height, spp;
  float rate;
  int32_t frames, accumulate, n_sparse, filter_fraction_bits;
};

void die(const char* what) { fprintf(stderr, "[ref_march_probe] %s\n", what); exit(2); }

template<typename T> void read_n(FILE* f, T* dst, size_t n)
{
  if (n && fread(dst, sizeof(T), n, f) != n) die("short scene file");
}

// compute_scalar_range (array.cpp:27-66: max from lowest(), min from max(), std::max / std::min) without tbb, followed by
// cuda_scalar_range (array.cpp:92-108): integers through the reference's integer_normalize<float, T>, floats cast
template<typename T> void scalar_range(const T* a, size_t n, float& lo, float& hi)
{
  T vmax = std::numeric_limits<T>::lowest(), vmin = std::numeric_limits<T>::max();
  for (size_t i = 0; i < n; ++i) {
    vmax = std::max(vmax, a[i]);
    vmin = std::min(vmin, a[i]);
  }
  if constexpr (std::is_integral<T>::value) {
    lo = integer_normalize<float, T>(vmin);
    hi = integer_normalize<float, T>(vmax);
  }
  else {
    lo = (float)vmin;
    hi = (float)vmax;
  }
}

// CreateArray3DScalarOptix7<T> (array.cpp:287-309): type, dims, normalised value range, scale; the texture is a shim descriptor
template<typename T> Array3DScalarOptix7 create_volume(const T* data, vec3i dims, OvrShimFormat format, OvrShimTexture& tex)
{
  Array3DScalarOptix7 out;
  out.type = value_type<T>();
  out.dims = dims;
  scalar_range<T>(data, (size_t)dims.x * dims.y * dims.z, out.lower.v, out.upper.v);
  out.scale.v = 1.f / (out.upper.v - out.lower.v);
  tex = OvrShimTexture{ data, format, { dims.x, dims.y, dims.z } };
  out.data = (cudaTextureObject_t)&tex;
  return out;
}

// convert_volume<IType, float> (array.cpp:68-90): static_cast per voxel
template<typename T> std::vector<float> to_float(const void* src, size_t n)
{
  std::vector<float> out(n);
  for (size_t i = 0; i < n; ++i) out[i] = static_cast<float>(((const T*)src)[i]);
  return out;
}

} // namespace

int main(int n_args, char** args)
{
  if (n_args != 3) die("usage: ref_march_probe <scene file> <output file>");
  FILE* f = fopen(args[1], "rb");
  if (!f) die("cannot open the scene file");
  Header h;
  read_n(f, &h, 1);
  if (h.magic != 0x4D52564F) die("bad magic");
  const ValueType vtype = (ValueType)h.value_type;
  const size_t n_voxels = (size_t)h.dims[0] * h.dims[1] * h.dims[2];
  std::vector<char> voxels(n_voxels * value_type_size(vtype));
  read_n(f, voxels.data(), voxels.size());
  std::vector<float> colors((size_t)h.n_colors * 3), alphas((size_t)h.n_alphas * 2);
  read_n(f, colors.data(), colors.size());
  read_n(f, alphas.data(), alphas.size());
  std::vector<int32_t> sparse((size_t)h.n_sparse * 2);
  read_n(f, sparse.data(), sparse.size());
  fclose(f);

  ovr_shim_set_filter_fraction_bits(h.filter_fraction_bits);

  // ---- DeviceOptix7::Impl::buildScene (device_impl.cpp:283-302) + StructuredRegularVolume::load_from_array3d_scalar (volume.cpp:181-191)
  DeviceStructuredRegularVolume dev; // what the hit programs see as `self`
  const vec3i dims(h.dims[0], h.dims[1], h.dims[2]);
  const vec3f grid_spacing(h.spacing[0], h.spacing[1], h.spacing[2]), grid_origin(h.origin[0], h.origin[1], h.origin[2]);
  const vec3f scale = grid_spacing * vec3f(dims);
  const affine3f matrix = affine3f::translate(grid_origin) * affine3f::scale(scale);
  OvrShimTexture volume_tex, color_tex, alpha_tex;
  std::vector<float> converted;
  switch (vtype) { // CreateArray3DScalarOptix7(array_3d_scalar_t), array.cpp:322-351
  case VALUE_TYPE_UINT8: dev.volume = create_volume<uint8_t>((const uint8_t*)voxels.data(), dims, OVR_SHIM_U8, volume_tex); break;
  case VALUE_TYPE_INT8: dev.volume = create_volume<int8_t>((const int8_t*)voxels.data(), dims, OVR_SHIM_I8, volume_tex); break;
  case VALUE_TYPE_UINT32: dev.volume = create_volume<uint32_t>((const uint32_t*)voxels.data(), dims, OVR_SHIM_U32, volume_tex); break;
  case VALUE_TYPE_INT32: dev.volume = create_volume<int32_t>((const int32_t*)voxels.data(), dims, OVR_SHIM_I32, volume_tex); break;
  case VALUE_TYPE_FLOAT: dev.volume = create_volume<float>((const float*)voxels.data(), dims, OVR_SHIM_F32, volume_tex); break;
  case VALUE_TYPE_UINT16: converted = to_float<uint16_t>(voxels.data(), n_voxels); break;
  case VALUE_TYPE_INT16: converted = to_float<int16_t>(voxels.data(), n_voxels); break;
  case VALUE_TYPE_DOUBLE: converted = to_float<double>(voxels.data(), n_voxels); break;
  default: die("unexpected volume type");
  }
  if (!converted.empty()) dev.volume = create_volume<float>(converted.data(), dims, OVR_SHIM_F32, volume_tex);
  const vec2f original_value_range(dev.volume.lower.v, dev.volume.upper.v);
  // StructuredRegularVolume::set_value_range (volume.cpp:131-154); at load time it is called with the invalid range (1, -1)
  auto set_value_range = [&](float lo, float hi) {
    Array3DScalarOptix7& v = dev.volume;
    if (hi >= lo) { // a valid range replaces the data range, normalised the way the voxels are
      v.upper.v = integer_normalize(hi, v.type);
      v.lower.v = integer_normalize(lo, v.type);
    }
    v.scale.v = 1.f / (v.upper.v - v.lower.v);
    dev.tfn.value_range = vec2f(max(original_value_range.x, v.lower.v), min(original_value_range.y, v.upper.v)); // only the path tracer reads these
    dev.tfn.range_rcp_norm = 1.f / (dev.tfn.value_range.y - dev.tfn.value_range.x);
  };
  set_value_range(1.f, -1.f);

  // ---- set_transfer_function(colors, alphas, range) (volume.cpp:110-129, 82-102; device_impl.cpp:146-153): rgb triples become
  // vec4f(r, g, b, 1), alphas take the second float of every (position, alpha) pair; CreateArray1D*Optix7 (array.cpp:116-141, 217-245)
  std::vector<vec4f> tfn_colors_data(colors.size() / 3);
  for (size_t i = 0; i < tfn_colors_data.size(); ++i) tfn_colors_data[i] = vec4f(colors[3 * i + 0], colors[3 * i + 1], colors[3 * i + 2], 1.f);
  std::vector<float> tfn_alphas_data(alphas.size() / 2);
  for (size_t i = 0; i < tfn_alphas_data.size(); ++i) tfn_alphas_data[i] = alphas[2 * i + 1];
  if (tfn_colors_data.empty() || tfn_alphas_data.empty()) die("empty transfer function");
  color_tex = OvrShimTexture{ tfn_colors_data.data(), OVR_SHIM_F32X4, { (int)tfn_colors_data.size(), 1, 1 } };
  alpha_tex = OvrShimTexture{ tfn_alphas_data.data(), OVR_SHIM_F32, { (int)tfn_alphas_data.size(), 1, 1 } };
  dev.tfn.color.type = VALUE_TYPE_FLOAT4;
  dev.tfn.color.dims = (int)tfn_colors_data.size();
  dev.tfn.color.data = (cudaTextureObject_t)&color_tex;
  dev.tfn.opacity.type = VALUE_TYPE_FLOAT;
  dev.tfn.opacity.dims = (int)tfn_alphas_data.size();
  dev.tfn.opacity.data = (cudaTextureObject_t)&alpha_tex;
  set_value_range(h.tfn_range[0], h.tfn_range[1]);

  // ---- set_sampling_rate + commit (volume.cpp:156-179): base stays 1, step = 1 / rate
  dev.base = 1.f;
  dev.step = 1.f / h.rate;

  // ---- the instance (device_impl.cpp:586-592, volume.cpp:25-40) and the shader binding table (device_impl.cpp:485-493)
  float transform[12];
  transform[0] = matrix.l.row0().x; transform[1] = matrix.l.row0().y; transform[2] = matrix.l.row0().z; transform[3] = matrix.p.x;
  transform[4] = matrix.l.row1().x; transform[5] = matrix.l.row1().y; transform[6] = matrix.l.row1().z; transform[7] = matrix.p.y;
  transform[8] = matrix.l.row2().x; transform[9] = matrix.l.row2().y; transform[10] = matrix.l.row2().z; transform[11] = matrix.p.z;
  const DeviceStructuredRegularVolume* dev_ptr = &dev; // the hit group's record holds a POINTER to the volume (get_program_data)
  ovr_shim_set_instance(transform, &dev_ptr, VISIBILITY_VOLUME);
  const OvrShimProgram is[2] = { __intersection__volume, __intersection__volume };
  const OvrShimProgram ch[2] = { __closesthit__volume_raymarching, __closesthit__volume_shadow };
  const OvrShimProgram ms[2] = { __miss__raymarching, __miss__shadow };
  ovr_shim_set_programs(2, is, ch, ms);

  // ---- DeviceOptix7::Impl::commit (device_impl.cpp:113-197): frame size, camera basis, flags
  LaunchParams& params = optix_launch_params;
  params.frame.size = vec2i(h.width, h.height);
  {
    const vec3f from(h.cam_from[0], h.cam_from[1], h.cam_from[2]), at(h.cam_at[0], h.cam_at[1], h.cam_at[2]), up(h.cam_up[0], h.cam_up[1], h.cam_up[2]);
    const float t = 2.f * tan(h.fovy * 0.5f * (float)M_PI / 180.f);
    const vec2i& size = params.frame.size;
    const float aspect = size.x / float(size.y);
    LaunchParams::DeviceCamera cam;
    cam.position = from;
    cam.direction = normalize(at - from);
    cam.horizontal = t * aspect * normalize(cross(cam.direction, up));
    cam.vertical = cross(cam.horizontal, cam.direction) / aspect;
    params.last_camera = LaunchParams::DeviceCamera(); // the first commit copies the still-empty camera; only the optical flow, which no frame holds, reads it
    params.camera = cam;
  }
  params.sample_per_pixel = h.spp;
  params.enable_path_tracing = false;
  params.enable_sparse_sampling = h.n_sparse > 0;
  params.enable_frame_accumulation = h.accumulate != 0;

  // ---- DeviceOptix7::Impl::render (device_impl.cpp:199-269), once per frame
  const size_t n_pixels = (size_t)h.width * h.height;
  std::vector<vec4f> rgba(n_pixels, vec4f(0.f)), accum_rgba(n_pixels, vec4f(0.f));
  std::vector<vec3f> grad(n_pixels, vec3f(0.f)), accum_grad(n_pixels, vec3f(0.f));
  params.frame.rgba = rgba.data();
  params.frame.grad = grad.data();
  params.frame_accum_rgba = accum_rgba.data();
  params.frame_accum_grad = accum_grad.data();
  params.frame_index = 0; // accumulation: reset to 0 before the first frame (:225-233); without: counts up from 0 all the same
  ovr_shim_reset_counters();
  for (int frame = 0; frame < h.frames; ++frame) {
    if (!params.enable_frame_accumulation && params.enable_sparse_sampling) { // framebuffer.reset() (:234-239)
      std::fill(rgba.begin(), rgba.end(), vec4f(0.f));
      std::fill(grad.begin(), grad.end(), vec3f(0.f));
    }
    params.frame_index++;
    params.frame.size_rcp = vec2f(1.f / (float)h.width, 1.f / (float)h.height); // vec2f(1) / vec2f(size), :242
    if (params.enable_sparse_sampling) { // createSparseSamples (:329-341): the launch is (number of listed pixels, 1, 1)
      params.sparse_sampling.xs_and_ys = sparse.data();
      for (int i = 0; i < h.n_sparse; ++i) {
        ovr_shim_set_launch_index((unsigned)i, 0);
        __raygen__render_frame();
      }
    }
    else {
      for (int iy = 0; iy < h.height; ++iy)
        for (int ix = 0; ix < h.width; ++ix) {
          ovr_shim_set_launch_index((unsigned)ix, (unsigned)iy);
          __raygen__render_frame();
        }
    }
  }

  uint64_t counters[2];
  ovr_shim_get_counters(counters);
  FILE* o = fopen(args[2], "wb");
  if (!o) die("cannot open the output file");
  fwrite(rgba.data(), sizeof(vec4f), n_pixels, o);
  fwrite(grad.data(), sizeof(vec3f), n_pixels, o);
  fwrite(counters, sizeof(uint64_t), 2, o);
  fwrite(&params.camera, sizeof(float), 12, o); // position, direction, horizontal, vertical: the camera as the shader is handed it
  fclose(o);
  return 0;
}
