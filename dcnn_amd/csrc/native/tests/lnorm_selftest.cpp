// Stand-alone self-test of the native channel-LayerNorm, LayerScale and GELU CPU kernels
// (cpu_ops.cpp layernorm_* / layer_scale_* / act_* code 6), float32 and float64, against naive
// loops in double. Built under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_lnorm_sanitizers.py: heap tensors sized exactly, so an index past a plane or the
// statistics is a sanitizer report. Host code only.
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
  long N, C, HW;
};

static unsigned g_state = 2468u;
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
static void run_layernorm(const Case& c, bool affine, double tol) {
  const long N = c.N, C = c.C, HW = c.HW;
  const size_t n = (size_t)N * C * HW, np = (size_t)N * HW;
  const double eps = 1e-6;
  std::vector<T> x(n), dy(n), gamma(C), beta(C);
  for (auto& v : x) v = (T)(rnd() + 0.25);
  for (auto& v : dy) v = (T)rnd();
  for (auto& v : gamma) v = (T)(1.0 + 0.5 * rnd());
  for (auto& v : beta) v = (T)rnd();
  auto at = [&](long b, long ch, long i) { return ((size_t)b * C + ch) * HW + i; };
  std::vector<double> yr(n), dxr(n), mr(np), rr(np), dgr(C, 0.5), dbr(C, -2.0);
  for (long b = 0; b < N; ++b)
    for (long i = 0; i < HW; ++i) {
      double s = 0, q = 0, m1 = 0, m2 = 0;
      for (long ch = 0; ch < C; ++ch) s += x[at(b, ch, i)];
      const double mean = s / C;
      for (long ch = 0; ch < C; ++ch) q += (x[at(b, ch, i)] - mean) * (x[at(b, ch, i)] - mean);
      const double rstd = 1.0 / std::sqrt(q / C + eps);
      mr[b * HW + i] = mean;
      rr[b * HW + i] = rstd;
      for (long ch = 0; ch < C; ++ch) {
        const double ga = affine ? (double)gamma[ch] : 1.0, be = affine ? (double)beta[ch] : 0.0;
        const double xh = (x[at(b, ch, i)] - mean) * rstd, d = dy[at(b, ch, i)];
        yr[at(b, ch, i)] = xh * ga + be;
        dgr[ch] += d * xh;
        dbr[ch] += d;
        m1 += d * ga;
        m2 += d * ga * xh;
      }
      m1 /= C;
      m2 /= C;
      for (long ch = 0; ch < C; ++ch) {
        const double ga = affine ? (double)gamma[ch] : 1.0;
        const double xh = (x[at(b, ch, i)] - mean) * rstd;
        dxr[at(b, ch, i)] = rstd * (dy[at(b, ch, i)] * ga - m1 - xh * m2);
      }
    }
  std::vector<T> y(n), dx(n), mean(np), rstd(np), dg(C, (T)0.5), db(C, (T)-2);
  layernorm_fwd<T>(x.data(), y.data(), N, C, HW, affine ? gamma.data() : nullptr, affine ? beta.data() : nullptr, eps,
                   mean.data(), rstd.data());
  CHECK(max_err(y, yr) < tol && max_err(mean, mr) < tol && max_err(rstd, rr) < tol);
  layernorm_bwd<T>(x.data(), dy.data(), mean.data(), rstd.data(), affine ? gamma.data() : nullptr, dx.data(),
                   affine ? dg.data() : nullptr, affine ? db.data() : nullptr, N, C, HW);
  // the saved statistics are rounded to T: the backward sees that rounding (float: ~1e-7 relative)
  CHECK(max_err(dx, dxr) < 20 * tol);
  if (affine) CHECK(max_err(dg, dgr) < 20 * tol && max_err(db, dbr) < 20 * tol);  // gradients accumulate
}

template <typename T>
static void run_layer_scale(const Case& c, double tol) {
  const long N = c.N, C = c.C, HW = c.HW;
  const size_t n = (size_t)N * C * HW;
  std::vector<T> x(n), dy(n), res(n), gamma(C);
  for (auto& v : x) v = (T)rnd();
  for (auto& v : dy) v = (T)rnd();
  for (auto& v : res) v = (T)rnd();
  for (auto& v : gamma) v = (T)rnd();
  std::vector<double> yr(n), y2r(n), dxr(n), dgr(C, 0.5);
  for (size_t k = 0; k < n; ++k) {
    const long ch = (long)((k / HW) % C);
    yr[k] = (double)gamma[ch] * x[k];
    y2r[k] = yr[k] + res[k];
    dxr[k] = (double)gamma[ch] * dy[k];
    dgr[ch] += (double)dy[k] * x[k];
  }
  std::vector<T> y(n), y2(n), dx(n), dg(C, (T)0.5), dg2(C, (T)0.5);
  layer_scale_fwd<T>(x.data(), gamma.data(), nullptr, y.data(), N, C, HW);
  layer_scale_fwd<T>(x.data(), gamma.data(), res.data(), y2.data(), N, C, HW);
  CHECK(max_err(y, yr) < tol && max_err(y2, y2r) < tol);
  layer_scale_bwd<T>(x.data(), dy.data(), gamma.data(), dx.data(), dg.data(), N, C, HW);
  CHECK(max_err(dx, dxr) < tol && max_err(dg, dgr) < tol);
  layer_scale_bwd<T>(x.data(), dy.data(), gamma.data(), nullptr, dg2.data(), N, C, HW);  // no input gradient
  CHECK(max_err(dg2, dgr) < tol);
}

template <typename T>
static void run_gelu(double tol) {
  const long n = 37;
  std::vector<T> x(n), dy(n), y(n), dx(n);
  std::vector<double> yr(n), dxr(n);
  for (long i = 0; i < n; ++i) {
    x[i] = (T)(-8.0 + 16.0 * i / (n - 1));
    dy[i] = (T)rnd();
    const double v = x[i], cdf = 0.5 * (1.0 + std::erf(v / std::sqrt(2.0)));
    yr[i] = v * cdf;
    dxr[i] = dy[i] * (cdf + v * std::exp(-0.5 * v * v) / std::sqrt(2.0 * M_PI));
  }
  act_fwd<T>(6, x.data(), y.data(), n, 0.0);
  act_bwd<T>(6, x.data(), dy.data(), dx.data(), n, 0.0);
  CHECK(max_err(y, yr) < tol && max_err(dx, dxr) < tol);
}

int main() {
  const Case cases[] = {
      {1, 8, 1},    // one position
      {2, 5, 3},    // odd channel count
      {3, 40, 6},   // more images than threads may take
      {2, 96, 4},   // a ConvNeXt width
      {4, 16, 1},   // a 2-D [N, F] input
  };
  for (const Case& c : cases) {
    for (bool affine : {false, true}) {
      run_layernorm<float>(c, affine, 2e-6);
      run_layernorm<double>(c, affine, 1e-13);
    }
    run_layer_scale<float>(c, 1e-6);
    run_layer_scale<double>(c, 1e-14);
  }
  run_gelu<float>(1e-6);
  run_gelu<double>(1e-14);
  std::printf("lnorm selftest OK\n");
  return 0;
}
