// max_depth_host.hpp - the host side of the depth limit (include/ovr_hip.h ovr_hip_set_max_depth; DESIGN.md section 26;
// open-volume-renderer_amd/max_depth.py is the normative text): what the setter accepts, which committed state draws a depth-limited frame, and
// OVR_HIP_MAX_DEPTH - a raw little-endian float32 file - as data.  Nothing here calls HIP: ovr_hip_api.cpp validates with it, host/frame.cpp and launch_plan.hpp
// decide the frame with it, the plugin reads its file with it, and tests/max_depth_host_driver.cpp holds it to the model on a machine without a GPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace ovrhip {

// the state as committed: the size of the image the renderer holds a device copy of; on = an image was set and not switched off
struct MaxDepthState {
  bool on = false;
  int width = 0, height = 0;
};

// what ovr_hip_set_max_depth accepts, in front of anything that changes: 0 = fine, else which rule refused (max_depth_rule_text).  depth == nullptr switches
// the limit off whatever the other arguments are.  The unit of a value is the march's own t - world length along the normalised ray from the ray's origin
enum MaxDepthRule { kMaxDepthOk = 0, kMaxDepthMemKind, kMaxDepthExtent, kMaxDepthOverflow };
constexpr size_t kMaxDepthPixels = (size_t)INT32_MAX; // the product as a 32-bit integer: a pixel index is a 32-bit number in every frame kernel
inline int max_depth_check(const void* depth, int mem_kind, long long width, long long height)
{
  if (!depth) return kMaxDepthOk;
  if (mem_kind != 0 && mem_kind != 1) return kMaxDepthMemKind; // OVR_HIP_MEM_HOST / OVR_HIP_MEM_DEVICE
  if (width < 1 || height < 1) return kMaxDepthExtent;
  if (width > (long long)INT32_MAX || height > (long long)INT32_MAX) return kMaxDepthOverflow;
  if ((unsigned long long)width > (unsigned long long)kMaxDepthPixels / (unsigned long long)height) return kMaxDepthOverflow;
  return kMaxDepthOk;
}
inline const char* max_depth_rule_text(int rule)
{
  switch (rule) {
  case kMaxDepthMemKind: return "bad mem_kind";
  case kMaxDepthExtent: return "width and height are at least 1";
  case kMaxDepthOverflow: return "width x height exceeds 2^31 - 1 pixels";
  default: return "";
  }
}

// which committed state draws a depth-limited frame: the committed frame is the march (march: no slices, isovalues or projection), the mode is on, the committed
// shading is NONE (0) or GRADIENT (1), neither pre-integration nor gradient opacity is active (their own rules said yes), and the image's size is the committed
// framebuffer's.  Otherwise the image is kept and not drawn
constexpr bool max_depth_active(bool on, bool march, int shading, bool preintegrated, bool gradient_opacity, bool size_matches)
{
  return on && march && (shading == 0 || shading == 1) && !preintegrated && !gradient_opacity && size_matches;
}
constexpr bool max_depth_size_matches(const MaxDepthState& s, int fb_width, int fb_height) { return s.width == fb_width && s.height == fb_height; }

// the cut of one pixel sample as the kernel forms it, for host-side checks: z < +inf is false for +inf and for NaN - no surface at this pixel
inline float max_depth_cut(float t1, float z)
{
  const bool limited = z < __builtin_inff();
  return limited ? (z < t1 ? z : t1) : t1;
}

// OVR_HIP_MAX_DEPTH as data: the bytes of a file as width * height little-endian float32 values in the frame's pixel order.  false - an error, never a
// shorter or padded image - unless the file holds exactly width * height * 4 bytes
inline bool max_depth_decode(const unsigned char* bytes, size_t n_bytes, int width, int height, std::vector<float>* out)
{
  if (!bytes || max_depth_check(bytes, 0, width, height) != kMaxDepthOk) return false;
  const size_t n = (size_t)width * (size_t)height;
  if (n_bytes != n * 4) return false;
  if (out) {
    out->resize(n);
    for (size_t i = 0; i < n; ++i) {
      const unsigned char* p = bytes + 4 * i;
      const uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
      float f;
      std::memcpy(&f, &u, 4);
      (*out)[i] = f;
    }
  }
  return true;
}

// the file behind OVR_HIP_MAX_DEPTH: false where it cannot be read or max_depth_decode refuses its size
inline bool max_depth_read_file(const char* path, int width, int height, std::vector<float>* out)
{
  if (!path || !*path || max_depth_check(path, 0, width, height) != kMaxDepthOk) return false;
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  const size_t want = (size_t)width * (size_t)height * 4;
  std::vector<unsigned char> bytes(want + 1); // (one more: a longer file reads past `want` and is refused)
  const size_t got = std::fread(bytes.data(), 1, want + 1, f);
  std::fclose(f);
  return max_depth_decode(bytes.data(), got, width, height, out);
}

} // namespace ovrhip
