// Stand-alone self-test of the native grouped-convolution CPU kernels (cpu_ops.cpp
// grouped_conv2d_fwd / grouped_conv2d_bwd), float32 and float64, against naive loops in double.
// Built under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_gconv_sanitizers.py: heap tensors sized exactly, so an index past a plane, a group or
// the padded border is a sanitizer report. Host code only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cpu_kernels.h"

using namespace dcnn_native::cpu;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

struct Case {
  int N, C, Co, G, H, W, KH, KW, SH, SW, PH, PW;
};

static unsigned g_state = 12345u;
static double rnd() {
  g_state = g_state * 1664525u + 1013904223u;
  return ((g_state >> 8) & 0xffff) / 32768.0 - 1.0;
}

template <typename T>
static double max_err(const std::vector<T>& a, const std::vector<double>& r) {
  double e = 0, m = 1e-30;
  for (size_t i = 0; i < r.size(); ++i) {
    e = std::fmax(e, std::fabs((double)a[i] - r[i]));
    m = std::fmax(m, std::fabs(r[i]));
  }
  return e / m;
}

template <typename T>
static void run(const Case& c, double tol) {
  const int OH = (c.H + 2 * c.PH - c.KH) / c.SH + 1, OW = (c.W + 2 * c.PW - c.KW) / c.SW + 1;
  const int Cig = c.C / c.G, Cog = c.Co / c.G;
  const size_t nx = (size_t)c.N * c.C * c.H * c.W, ny = (size_t)c.N * c.Co * OH * OW;
  const size_t nw = (size_t)c.Co * Cig * c.KH * c.KW;
  std::vector<T> x(nx), w(nw), b(c.Co), dy(ny);
  for (auto& v : x) v = (T)rnd();
  for (auto& v : w) v = (T)rnd();
  for (auto& v : b) v = (T)rnd();
  for (auto& v : dy) v = (T)rnd();
  // naive reference in double
  std::vector<double> yr(ny), dxr(nx, 0.0), dwr(nw, 0.0), dbr(c.Co, 0.0);
  for (int n = 0; n < c.N; ++n)
    for (int co = 0; co < c.Co; ++co)
      for (int oy = 0; oy < OH; ++oy)
        for (int ox = 0; ox < OW; ++ox) {
          const size_t yi = (((size_t)n * c.Co + co) * OH + oy) * OW + ox;
          double s = b[co];
          dbr[co] += dy[yi];
          for (int cl = 0; cl < Cig; ++cl)
            for (int ky = 0; ky < c.KH; ++ky)
              for (int kx = 0; kx < c.KW; ++kx) {
                const int iy = oy * c.SH + ky - c.PH, ix = ox * c.SW + kx - c.PW;
                if (iy < 0 || iy >= c.H || ix < 0 || ix >= c.W) continue;
                const size_t xi = (((size_t)n * c.C + (co / Cog) * Cig + cl) * c.H + iy) * c.W + ix;
                const size_t wi = (((size_t)co * Cig + cl) * c.KH + ky) * c.KW + kx;
                s += (double)w[wi] * x[xi];
                dxr[xi] += (double)w[wi] * dy[yi];
                dwr[wi] += (double)x[xi] * dy[yi];
              }
          yr[yi] = s;
        }
  std::vector<T> y(ny), dx(nx), dw(nw, (T)0.5), db(c.Co, (T)-2);
  grouped_conv2d_fwd<T>(x.data(), w.data(), b.data(), y.data(), c.N, c.C, c.H, c.W, c.Co, c.G, c.KH, c.KW, c.SH, c.SW,
                        c.PH, c.PW);
  CHECK(max_err(y, yr) < tol);
  grouped_conv2d_bwd<T>(x.data(), w.data(), dy.data(), dx.data(), dw.data(), db.data(), c.N, c.C, c.H, c.W, c.Co, c.G,
                        c.KH, c.KW, c.SH, c.SW, c.PH, c.PW);
  for (auto& v : dwr) v += 0.5;  // the parameter gradients accumulate
  for (auto& v : dbr) v -= 2.0;
  CHECK(max_err(dx, dxr) < tol && max_err(dw, dwr) < tol && max_err(db, dbr) < tol);
  // no bias, no input gradient, no bias gradient
  std::vector<T> y0(ny), dw0(nw, (T)0.5);
  grouped_conv2d_fwd<T>(x.data(), w.data(), nullptr, y0.data(), c.N, c.C, c.H, c.W, c.Co, c.G, c.KH, c.KW, c.SH, c.SW,
                        c.PH, c.PW);
  for (size_t i = 0; i < ny; ++i) yr[i] -= b[(i / ((size_t)OH * OW)) % c.Co];
  CHECK(max_err(y0, yr) < tol);
  grouped_conv2d_bwd<T>(x.data(), w.data(), dy.data(), nullptr, dw0.data(), nullptr, c.N, c.C, c.H, c.W, c.Co, c.G,
                        c.KH, c.KW, c.SH, c.SW, c.PH, c.PW);
  CHECK(max_err(dw0, dwr) < tol);
}

int main() {
  const Case cases[] = {
      {1, 8, 16, 2, 1, 1, 3, 3, 1, 1, 1, 1},    // one pixel: every tap but the centre is padding
      {2, 32, 32, 8, 5, 7, 3, 3, 1, 1, 1, 1},   // 4 channels per group
      {2, 24, 12, 3, 9, 9, 3, 3, 2, 2, 1, 1},   // G = 3, Co < Ci, stride 2 on an odd map
      {2, 16, 32, 2, 10, 6, 1, 3, 1, 2, 0, 1},  // rectangular kernel, stride and pad
      {3, 12, 12, 4, 8, 8, 3, 3, 2, 2, 0, 0},   // last input row and column unused
      {2, 8, 8, 2, 6, 5, 5, 5, 1, 1, 2, 2},     // 25 taps
  };
  for (const Case& c : cases) {
    run<float>(c, 1e-5);
    run<double>(c, 1e-12);
  }
  std::printf("gconv selftest OK\n");
  return 0;
}
