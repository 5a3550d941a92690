// depth_output_host.hpp - the host side of the depth layer (include/ovr_hip.h ovr_hip_set_depth_output; DESIGN.md section 27;
// open-volume-renderer_amd/depth_output.py is the normative text): what the setter accepts, which committed state draws a depth frame, and
// OVR_HIP_DEPTH_OUTPUT_FILE - a raw little-endian float32 file, the format OVR_HIP_MAX_DEPTH reads - as data.  Nothing here calls HIP: ovr_hip_api.cpp
// validates with it, host/frame.cpp and launch_plan.hpp decide the frame with it, the plugin writes its file with it, and tests/depth_output_host_driver.cpp
// holds it to the model and to max_depth_decode on a machine without a GPU.
#pragma once

#include "max_depth_host.hpp"

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace ovrhip {

constexpr int kDepthOutputOff = 0, kDepthOutputOn = 1; // OVR_HIP_DEPTH_OUTPUT_OFF / OVR_HIP_DEPTH_OUTPUT_ON
constexpr float kDepthOutputMaxThreshold = 0.9999f;    // the march's early-termination literal: above it a crossing could only happen by overshoot

// the state as committed
struct DepthOutputState {
  int mode = kDepthOutputOff;
  float threshold = 0.f; // tau, in (0, 0.9999f] while the mode is ON; 0 in mode OFF
};

// what ovr_hip_set_depth_output accepts, in front of anything that changes: 0 = fine, else which rule refused (depth_output_rule_text).  Mode OFF does not
// read the threshold
enum DepthOutputRule { kDepthOutputOk = 0, kDepthOutputMode, kDepthOutputThreshold };
inline int depth_output_check(int mode, float threshold)
{
  if (mode != kDepthOutputOff && mode != kDepthOutputOn) return kDepthOutputMode;
  if (mode == kDepthOutputOff) return kDepthOutputOk;
  if (!(threshold > 0.f) || !(threshold <= kDepthOutputMaxThreshold)) return kDepthOutputThreshold; // (NaN fails both comparisons)
  return kDepthOutputOk;
}
inline const char* depth_output_rule_text(int rule)
{
  switch (rule) {
  case kDepthOutputMode: return "unknown mode";
  case kDepthOutputThreshold: return "the threshold lies in (0, 0.9999]";
  default: return "";
  }
}

// which committed state draws a depth frame: the committed frame is the march (march: no slices, isovalues or projection), the mode is ON, the committed
// shading is NONE (0) or GRADIENT (1), and neither pre-integration nor gradient opacity is active (their own rules said yes).  Otherwise the setting is kept
// and not drawn.  The depth limit does not enter: a committed image of the framebuffer's size is applied by the depth frame (depth_output_limited)
constexpr bool depth_output_active(bool on, bool march, int shading, bool preintegrated, bool gradient_opacity)
{
  return on && march && (shading == 0 || shading == 1) && !preintegrated && !gradient_opacity;
}
// a depth frame applies the depth limit iff the depth limit's own rule draws it (max_depth_active over the same committed state)
constexpr bool depth_output_limited(bool active, bool max_depth_on, bool size_matches) { return active && max_depth_on && size_matches; }

// OVR_HIP_DEPTH_OUTPUT as data: one number and nothing behind it, a threshold the setter accepts.  false - an error, never a default - otherwise
inline bool parse_depth_output(const char* text, float* threshold)
{
  if (!text || !*text) return false;
  char* end = nullptr;
  const float t = std::strtof(text, &end);
  if (end == text || *end != '\0' || depth_output_check(kDepthOutputOn, t) != kDepthOutputOk) return false;
  if (threshold) *threshold = t;
  return true;
}

// what a finished pixel's layer (d_sum, S, share) resolves to as a threshold depth: d_sum / share where share > 0, +inf - the depth limit's "no surface" -
// elsewhere.  depth_output.resolve is the numpy text
inline float depth_output_threshold_depth(float d_sum, float share) { return share > 0.f ? d_sum / share : __builtin_inff(); }

// OVR_HIP_DEPTH_OUTPUT_FILE as data: n float32 values as 4 n little-endian bytes, in the order given - the inverse of max_depth_decode
inline void depth_output_encode(const float* values, size_t n, std::vector<unsigned char>* out)
{
  out->resize(4 * n);
  for (size_t i = 0; i < n; ++i) {
    uint32_t u;
    std::memcpy(&u, values + i, 4);
    unsigned char* p = out->data() + 4 * i;
    p[0] = (unsigned char)(u & 0xffu); p[1] = (unsigned char)((u >> 8) & 0xffu); p[2] = (unsigned char)((u >> 16) & 0xffu); p[3] = (unsigned char)((u >> 24) & 0xffu);
  }
}

// the file behind OVR_HIP_DEPTH_OUTPUT_FILE: the resolved threshold depth of a frame's layer (3 floats per pixel: d_sum, S, share), width * height values in
// the frame's pixel order.  false where the size is one the depth limit refuses or the file cannot be written whole
inline bool depth_output_write_file(const char* path, const float* layer, int width, int height)
{
  if (!path || !*path || !layer || max_depth_check(layer, 0, width, height) != kMaxDepthOk) return false;
  const size_t n = (size_t)width * (size_t)height;
  std::vector<float> depth(n);
  for (size_t i = 0; i < n; ++i) depth[i] = depth_output_threshold_depth(layer[3 * i], layer[3 * i + 2]);
  std::vector<unsigned char> bytes;
  depth_output_encode(depth.data(), n, &bytes);
  std::FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  const size_t put = std::fwrite(bytes.data(), 1, bytes.size(), f);
  return std::fclose(f) == 0 && put == bytes.size();
}

} // namespace ovrhip
