// Conv tap tables and kernel argument blocks (conv_args.cpp), shared by the Python front end
// (bindings.cpp, ops/hip.py) and the C++ host API's GPU backend (csrc/host/ops_gpu.hip): the step
// between "route chosen" (conv_route.cpp) and "kernel launched". One owner per table and per
// struct's tap / class fields; host code only. Included by api.h.
#pragma once
#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "api.h"

namespace dcnn {
// (row offset, column offset, source element offset, B-row element offset) of one kernel tap
using ConvTap = std::array<int, 4>;
using ConvTaps = std::vector<ConvTap>;
using WgradTaps = std::vector<std::array<int, 2>>;

// Forward conv: tap (ky, kx) reads x at (ky - PH, kx - PW). C: the channel count of the operand
// rows (the split-precision fp32 path gathers 3 * Ci wide rows).
ConvTaps conv_fwd_taps(const ConvRouteGeom& g, int C);
// Weight gradient: the (ky - PH, kx - PW) input offset of every tap.
WgradTaps conv_wgrad_taps(const ConvRouteGeom& g);
// Data gradient by stride phases: input pixels (ry + SH * i, rx + SW * j) form a GH x GW grid that
// is a dense conv of dy over the taps with (ry + PH - ky) % SH == 0 and (rx + PW - kx) % SW == 0,
// read at dy offset ((ry + PH - ky) / SH, (rx + PW - kx) / SW). Every phase with GH, GW > 0, in
// (ry, rx) order, owns taps [t0, t0 + nt) of one flat table (nt = 0: no tap reaches the phase);
// source offsets index dy rows of Co channels, B-row offsets the transposed weight [C][T][Co].
// Stride 1 is the single phase of all taps flipped: the halo data gradient's table.
struct DgradPhase { int ry, rx, GH, GW, t0, nt; };
struct DgradPhases {
  std::vector<DgradPhase> phases;
  ConvTaps taps;
};
DgradPhases conv_dgrad_phases(const ConvRouteGeom& g);

// ---- tap (and row class) fields of the argument structs; `who` names the caller in the error
inline void set_taps(G2Args& a, const ConvTaps& t, const char* who) {
  if (t.size() > 64) throw std::runtime_error(std::string(who) + ": more than 64 taps");
  a.ntaps = (int)t.size();
  for (size_t i = 0; i < t.size(); ++i) {
    a.tap_dy[i] = t[i][0]; a.tap_dx[i] = t[i][1]; a.tap_srcoff[i] = t[i][2]; a.tap_b[i] = t[i][3];
  }
}
// row classes of a grouped launch, (first tap, taps, ORY, ORX) each; M rows in all (none: one class)
inline void set_classes(G2Args& a, const std::vector<std::array<int, 4>>& c, const char* who) {
  if (c.size() > 4) throw std::runtime_error(std::string(who) + ": at most 4 row classes");
  a.ncls = (int)c.size();
  a.cls_rows = c.empty() ? 0 : a.M / (int)c.size();
  for (size_t k = 0; k < c.size(); ++k) {
    a.cls_t0[k] = c[k][0]; a.cls_nt[k] = c[k][1]; a.cls_ory[k] = c[k][2]; a.cls_orx[k] = c[k][3];
  }
}
inline void set_taps(HConvArgs& a, const ConvTaps& t, const char* who) {  // (source offsets unused)
  if (t.size() > 9 || t.empty()) throw std::runtime_error(std::string(who) + ": 1..9 taps");
  a.ntaps = (int)t.size();
  for (size_t i = 0; i < t.size(); ++i) { a.tap_dy[i] = t[i][0]; a.tap_dx[i] = t[i][1]; a.tap_b[i] = t[i][3]; }
}
inline void set_taps(HWArgs& a, const WgradTaps& t, const char* who) {
  if (t.size() > 9 || t.empty()) throw std::runtime_error(std::string(who) + ": 1..9 taps");
  a.ntaps = (int)t.size();
  for (size_t i = 0; i < t.size(); ++i) { a.tap_dy[i] = t[i][0]; a.tap_dx[i] = t[i][1]; }
}
inline void set_taps(T2Args& a, const WgradTaps& t, const char* who) {
  if (t.size() > 64) throw std::runtime_error(std::string(who) + ": more than 64 taps");
  a.ntaps = (int)t.size();
  for (size_t i = 0; i < t.size(); ++i) { a.tap_dy[i] = t[i][0]; a.tap_dx[i] = t[i][1]; }
}

// ---- whole argument blocks of a bf16 conv's launches (x / dy NHWC, w [Co][T][C], wt [C][T][Co])
G2Args g2_fwd_args(const void* x, const void* w, void* y, const float* bias, const ConvRouteGeom& g);
HConvArgs hconv_fwd_args(const void* x, const void* w, void* y, const float* bias, const ConvRouteGeom& g);
// halo data gradient of a stride-1 'same' conv: a 'same' conv of dy with the flipped taps
HConvArgs hconv_dgrad_args(const void* dy, const void* wt, void* dx, const void* residual, const ConvRouteGeom& g);
// every phase of p (equal GH x GW) as the row classes of one grouped launch; one phase: ungrouped.
// residual_compact: `residual` is [N][GH][GW][C], the gradient at the pixels (SH i, SW j) only (a
// strided 1x1 pad-0 shortcut's) and zero elsewhere: G2Args::res_cls = the class of phase (0, 0)
G2Args g2_dgrad_args(const void* dy, const void* wt, void* dx, const void* residual, const ConvRouteGeom& g,
                     const DgradPhases& p, bool residual_compact = false);
T2Args t2_wgrad_args(const void* dy, const void* x, float* slab, float* bias_slab, const ConvRouteGeom& g);
// hwgrad (stride 1 'same': the input grid) or, s2, hwgrad_s2 (3x3 stride 2: dY's grid, no tap table)
HWArgs hwgrad_args(const void* dy, const void* x, float* slab, float* bias_slab, const ConvRouteGeom& g, bool s2);
}  // namespace dcnn
