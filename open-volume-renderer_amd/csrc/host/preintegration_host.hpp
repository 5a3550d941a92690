// preintegration_host.hpp - the host side of pre-integrated classification (include/ovr_hip.h ovr_hip_set_preintegration; DESIGN.md section 24;
// open-volume-renderer_amd/preintegration.py is the normative text): how many nodes the integral table has, the table itself, and OVR_HIP_PREINTEGRATION as
// data.  Nothing here calls HIP: host/frame.cpp builds the table of the committed transfer function with it, launch_plan.hpp sizes the frame's LDS with it, and
// tests/preintegration_host_driver.cpp holds it to the model on a machine without a GPU.
//
// The table: M = S * max(n_alpha - 1, n_color - 1, 1) + 1 nodes at u_j = j / (M - 1).  At a node a_j = clamp01 of the alpha table's nodal lerp at u_j, c_j =
// clamp01 per channel of the colour table's, both in float64 from the float32 entries; tau_j = -log2(1 - min(a_j, 1 - 2^-24)); T_j and K_j (rgb) are the
// cumulative trapezoid sums of tau and tau * c over u.  A node is (T, Kr, Kg, Kb), summed in float64 and rounded ONCE to float32; the table carries one more
// entry, a copy of the last (the kernel reads nodes i0 and i0 + 1 without a min, as stage_tf's tables are read).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace ovrhip {

constexpr int kPreintegrationSubdivisions[3] = { 4, 2, 1 }; // S, the largest whose table fits the frame's LDS budget

// segments of the node table at subdivision 1: the finer of the two tables' (a one-entry pair still has one segment)
constexpr int preintegration_segments(int n_color, int n_alpha) { return std::max(std::max(n_alpha - 1, n_color - 1), 1); }
constexpr int preintegration_nodes(int n_color, int n_alpha, int subdivision) { return subdivision * preintegration_segments(n_color, n_alpha) + 1; }
// bytes of the table as the kernel stages it: M + 1 float4s
constexpr size_t preintegration_table_bytes(int nodes) { return (size_t)16 * ((size_t)nodes + 1); }
// the largest of 4, 2, 1 whose table fits in `room` bytes; 0: not even S = 1 fits (the frame is an error)
constexpr int preintegration_subdivision(int n_color, int n_alpha, size_t room)
{
  for (int s : kPreintegrationSubdivisions)
    if (preintegration_table_bytes(preintegration_nodes(n_color, n_alpha, s)) <= room) return s;
  return 0;
}

namespace preintegration_detail {
inline double clamp01(double x) { return x < 0.0 ? 0.0 : x > 1.0 ? 1.0 : (x == x ? x : 0.0); } // (a NaN entry reads 0, as the kernels' clamp01 has it)
// the nodal lerp of an n-entry table (stride floats apart) at u in [0, 1], in float64: x = u * (n - 1), i0 = floor(x), clamp-to-edge pair (i0, min(i0 + 1, n - 1))
inline double table_lerp(const float* t, int n, int stride, double u)
{
  const double x = u * (double)(n - 1);
  int i0 = (int)x;
  if (i0 > n - 1) i0 = n - 1;
  const int i1 = std::min(i0 + 1, n - 1);
  const double f = x - (double)i0;
  const double a = (double)t[(size_t)i0 * stride], b = (double)t[(size_t)i1 * stride];
  return a + f * (b - a);
}
} // namespace preintegration_detail

// the node table of a transfer function: colours as n_color float4s (rgb read, stride 4 - the staging layout of upload_tfn) and n_alpha alphas.  out: 4 * (M + 1)
// floats.  Returns M; 0 (out untouched) for an empty table or a subdivision below 1
inline int build_preintegration_nodes(const float* colors_rgba, int n_color, const float* alphas, int n_alpha, int subdivision, std::vector<float>& out)
{
  using namespace preintegration_detail;
  if (!colors_rgba || !alphas || n_color < 1 || n_alpha < 1 || subdivision < 1) return 0;
  const int M = preintegration_nodes(n_color, n_alpha, subdivision);
  const double h = 1.0 / (double)(M - 1);
  const double a_max = 1.0 - 5.9604644775390625e-08; // 1 - 2^-24: tau stays finite (24 at the most)
  out.assign((size_t)4 * ((size_t)M + 1), 0.f);
  double T = 0.0, K[3] = { 0.0, 0.0, 0.0 };
  double tau0 = 0.0, c0[3] = { 0.0, 0.0, 0.0 };
  for (int j = 0; j < M; ++j) {
    const double u = (double)j / (double)(M - 1);
    const double a = clamp01(table_lerp(alphas, n_alpha, 1, u));
    const double tau = -std::log2(1.0 - std::min(a, a_max));
    double c[3];
    for (int ch = 0; ch < 3; ++ch) c[ch] = clamp01(table_lerp(colors_rgba + ch, n_color, 4, u));
    if (j > 0) {
      T += 0.5 * (tau0 + tau) * h;
      for (int ch = 0; ch < 3; ++ch) K[ch] += 0.5 * (tau0 * c0[ch] + tau * c[ch]) * h;
    }
    out[(size_t)4 * j + 0] = (float)T;
    for (int ch = 0; ch < 3; ++ch) out[(size_t)4 * j + 1 + ch] = (float)K[ch];
    tau0 = tau;
    for (int ch = 0; ch < 3; ++ch) c0[ch] = c[ch];
  }
  for (int k = 0; k < 4; ++k) out[(size_t)4 * M + k] = out[(size_t)4 * (M - 1) + k];
  return M;
}

// OVR_HIP_PREINTEGRATION as data: "0" -> OFF, "1" -> SEGMENTS, the whole string; false for anything else - an empty string, white space, trailing text,
// another number - an error, never a default the user did not write.  Unset (a null pointer) is not parsed: the plugin calls nothing
inline bool parse_preintegration(const char* text, int* mode)
{
  if (!text || (text[0] != '0' && text[0] != '1') || text[1] != 0) return false;
  if (mode) *mode = text[0] - '0';
  return true;
}

} // namespace ovrhip
