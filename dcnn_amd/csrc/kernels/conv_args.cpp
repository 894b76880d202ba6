// Conv tap tables and kernel argument blocks, shared by both front ends (see conv_args.h): like
// the routing table (conv_route.cpp), one place computes them, so the Python front end and the
// C++ host API hand the kernels the same index arithmetic.
#include "conv_args.h"

namespace dcnn {

ConvTaps conv_fwd_taps(const ConvRouteGeom& g, int C) {
  ConvTaps taps;
  for (int ky = 0; ky < g.KH; ++ky)
    for (int kx = 0; kx < g.KW; ++kx) {
      const int dy = ky - g.PH, dx = kx - g.PW;
      taps.push_back({dy, dx, (dy * g.W + dx) * C, (ky * g.KW + kx) * C});
    }
  return taps;
}

WgradTaps conv_wgrad_taps(const ConvRouteGeom& g) {
  WgradTaps taps;
  for (int ky = 0; ky < g.KH; ++ky)
    for (int kx = 0; kx < g.KW; ++kx) taps.push_back({ky - g.PH, kx - g.PW});
  return taps;
}

DgradPhases conv_dgrad_phases(const ConvRouteGeom& g) {
  DgradPhases p;
  for (int ry = 0; ry < g.SH; ++ry)
    for (int rx = 0; rx < g.SW; ++rx) {
      const int GH = (g.H - ry + g.SH - 1) / g.SH, GW = (g.W - rx + g.SW - 1) / g.SW;
      if (GH <= 0 || GW <= 0) continue;
      DgradPhase c{ry, rx, GH, GW, (int)p.taps.size(), 0};
      // (the remainder is tested before the division, so a negative numerator divides exactly)
      for (int ky = 0; ky < g.KH; ++ky) {
        if ((ry + g.PH - ky) % g.SH) continue;
        const int dyo = (ry + g.PH - ky) / g.SH;
        for (int kx = 0; kx < g.KW; ++kx) {
          if ((rx + g.PW - kx) % g.SW) continue;
          const int dxo = (rx + g.PW - kx) / g.SW;
          p.taps.push_back({dyo, dxo, (dyo * g.OW + dxo) * g.Co, (ky * g.KW + kx) * g.Co});
          ++c.nt;
        }
      }
      p.phases.push_back(c);
    }
  return p;
}

namespace {
unsigned bytes16(long elems) { return (unsigned)(elems * 2); }
long x_elems(const ConvRouteGeom& g) { return (long)g.N * g.H * g.W * g.C; }
long y_elems(const ConvRouteGeom& g) { return (long)g.N * g.OH * g.OW * g.Co; }
long w_elems(const ConvRouteGeom& g) { return (long)g.Co * g.KH * g.KW * g.C; }
}  // namespace

G2Args g2_fwd_args(const void* x, const void* w, void* y, const float* bias, const ConvRouteGeom& g) {
  G2Args a{};
  a.A = static_cast<const bf16*>(x); a.B = static_cast<const bf16*>(w); a.C = static_cast<bf16*>(y);
  a.a_bytes = bytes16(x_elems(g)); a.b_bytes = bytes16(w_elems(g));
  a.M = g.N * g.OH * g.OW; a.N = g.Co; a.Cs = g.C;
  a.H = g.H; a.W = g.W; a.GH = g.OH; a.GW = g.OW; a.SY = g.SH; a.SX = g.SW;
  set_taps(a, conv_fwd_taps(g, g.C), "conv_fwd");
  a.ldb = g.KH * g.KW * g.C; a.ldc = g.Co;
  a.OH = g.OH; a.OW = g.OW; a.OSY = 1; a.OSX = 1; a.ORY = 0; a.ORX = 0;
  a.bias = bias;
  return a;
}

HConvArgs hconv_fwd_args(const void* x, const void* w, void* y, const float* bias, const ConvRouteGeom& g) {
  HConvArgs a{};
  a.A = static_cast<const bf16*>(x); a.B = static_cast<const bf16*>(w); a.C = static_cast<bf16*>(y);
  a.a_bytes = bytes16(x_elems(g)); a.b_bytes = bytes16(w_elems(g));
  a.NB = g.N; a.H = g.H; a.W = g.W; a.Cs = g.C; a.N = g.Co; a.ldb = g.KH * g.KW * g.C;
  set_taps(a, conv_fwd_taps(g, g.C), "conv_fwd");
  a.bias = bias;
  return a;
}

HConvArgs hconv_dgrad_args(const void* dy, const void* wt, void* dx, const void* residual, const ConvRouteGeom& g) {
  HConvArgs a{};
  a.A = static_cast<const bf16*>(dy); a.B = static_cast<const bf16*>(wt); a.C = static_cast<bf16*>(dx);
  a.a_bytes = bytes16(y_elems(g)); a.b_bytes = bytes16(w_elems(g));
  a.NB = g.N; a.H = g.OH; a.W = g.OW; a.Cs = g.Co; a.N = g.C; a.ldb = g.KH * g.KW * g.Co;
  set_taps(a, conv_dgrad_phases(g).taps, "conv_dgrad");
  a.residual = static_cast<const bf16*>(residual);
  return a;
}

G2Args g2_dgrad_args(const void* dy, const void* wt, void* dx, const void* residual, const ConvRouteGeom& g,
                     const DgradPhases& p, bool residual_compact) {
  const DgradPhase& c0 = p.phases.at(0);
  G2Args a{};
  a.A = static_cast<const bf16*>(dy); a.B = static_cast<const bf16*>(wt); a.C = static_cast<bf16*>(dx);
  a.a_bytes = bytes16(y_elems(g)); a.b_bytes = bytes16(w_elems(g));
  a.M = (int)((long)g.N * c0.GH * c0.GW * (long)p.phases.size()); a.N = g.C; a.Cs = g.Co;
  a.H = g.OH; a.W = g.OW; a.GH = c0.GH; a.GW = c0.GW; a.SY = 1; a.SX = 1;
  set_taps(a, p.taps, "conv_dgrad");
  a.ldb = g.KH * g.KW * g.Co; a.ldc = g.C;
  a.OH = g.H; a.OW = g.W; a.OSY = g.SH; a.OSX = g.SW; a.ORY = c0.ry; a.ORX = c0.rx;
  a.residual = static_cast<const bf16*>(residual);
  if (p.phases.size() > 1) {
    std::vector<std::array<int, 4>> cls;
    for (const DgradPhase& c : p.phases) cls.push_back({c.t0, c.nt, c.ry, c.rx});
    set_classes(a, cls, "conv_dgrad");
  }
  if (residual_compact) {
    // the residual covers the pixels (SH i, SW j) only: the phase (ry, rx) = (0, 0), as its class
    if (residual == nullptr || p.phases.size() < 2)
      throw std::runtime_error("conv_dgrad: a phase-compact residual needs a strided grouped launch and a residual");
    for (size_t k = 0; k < p.phases.size(); ++k)
      if (p.phases[k].ry == 0 && p.phases[k].rx == 0) a.res_cls = (int)k;
    if (a.res_cls < 0 || p.phases[a.res_cls].nt < 1)
      throw std::runtime_error("conv_dgrad: no tap reaches the phase (0, 0) of a phase-compact residual");
  }
  return a;
}

T2Args t2_wgrad_args(const void* dy, const void* x, float* slab, float* bias_slab, const ConvRouteGeom& g) {
  T2Args a{};
  a.dY = static_cast<const bf16*>(dy); a.X = static_cast<const bf16*>(x); a.slab = slab; a.bias_slab = bias_slab;
  a.a_bytes = bytes16(y_elems(g)); a.b_bytes = bytes16(x_elems(g));
  a.M = g.Co; a.N = g.KH * g.KW * g.C; a.P = g.N * g.OH * g.OW; a.ldy = g.Co; a.Cs = g.C;
  a.H = g.H; a.W = g.W; a.GH = g.OH; a.GW = g.OW; a.SY = g.SH; a.SX = g.SW;
  set_taps(a, conv_wgrad_taps(g), "conv_wgrad");
  return a;
}

HWArgs hwgrad_args(const void* dy, const void* x, float* slab, float* bias_slab, const ConvRouteGeom& g, bool s2) {
  HWArgs a{};
  a.dY = static_cast<const bf16*>(dy); a.X = static_cast<const bf16*>(x); a.slab = slab; a.bias_slab = bias_slab;
  a.dy_bytes = bytes16(y_elems(g)); a.x_bytes = bytes16(x_elems(g));
  a.NB = g.N; a.H = s2 ? g.OH : g.H; a.W = s2 ? g.OW : g.W; a.Cs = g.C; a.Co = g.Co;
  if (s2)
    a.ntaps = 9;
  else
    set_taps(a, conv_wgrad_taps(g), "conv_wgrad");
  return a;
}

}  // namespace dcnn
