// Stand-alone self-test of the native stochastic-depth and weight-decay-exclusion CPU kernels
// (cpu_ops.cpp drop_path_mask / drop_path_scale / adam_step_nodecay), float32 and float64, against
// naive loops. Built under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_drop_path_sanitizers.py: heap buffers sized exactly (the mask N floats, the block
// table one byte per 64 elements), so an index past a sample, the mask or the table is a sanitizer
// report. Host code only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
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

static unsigned g_state = 97531u;
static double rnd() {
  g_state = g_state * 1664525u + 1013904223u;
  return ((g_state >> 8) & 0xffff) / 32768.0 - 1.0;
}

static void run_mask() {
  const uint64_t seeds[] = {1ull, (1ull << 40) + 3ull, ~0ull};
  for (uint64_t seed : seeds)
    for (uint64_t draw : {1ull, 2ull, 1000ull})
      for (long N : {1l, 3l, 4l, 5l, 257l}) {
        std::vector<float> m((size_t)N, -1.f), longer((size_t)N + 7, -1.f);
        drop_path_mask(m.data(), N, 0.5, seed, draw);
        drop_path_mask(longer.data(), N + 7, 0.5, seed, draw);
        for (long n = 0; n < N; ++n) {
          CHECK(m[n] == 0.f || m[n] == 2.f);
          CHECK(m[n] == longer[n]);  // m[n] does not depend on N
        }
      }
  // the keep share: N = 4096, p = 0.25, within 0.75 +- 0.04 (6 sigma of Binomial(4096, 0.75))
  std::vector<float> m(4096);
  drop_path_mask(m.data(), 4096, 0.25, 20240607ull, 1);
  long kept = 0;
  const float keep = 1.0f / (1.0f - 0.25f);
  for (float v : m) {
    CHECK(v == 0.f || v == keep);
    kept += v != 0.f;
  }
  CHECK(std::fabs(kept / 4096.0 - 0.75) <= 0.04);
  // consecutive draws differ
  std::vector<float> a(64), b(64);
  drop_path_mask(a.data(), 64, 0.5, 7, 1);
  drop_path_mask(b.data(), 64, 0.5, 7, 2);
  CHECK(a != b);
  bool threw = false;
  try {
    drop_path_mask(a.data(), 64, 1.0, 7, 1);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
}

template <typename T>
static void run_scale(long N, long row) {
  const size_t n = (size_t)N * row;
  std::vector<T> x(n), y(n, (T)7);
  for (auto& v : x) v = (T)rnd();
  std::vector<float> m((size_t)N);
  drop_path_mask(m.data(), N, 0.5, 11, 3);
  drop_path_scale<T>(x.data(), m.data(), y.data(), N, row);
  for (long s = 0; s < N; ++s)
    for (long i = 0; i < row; ++i) CHECK(y[s * row + i] == (T)m[s] * x[s * row + i]);
}

// flat buffer of `n` elements (a multiple of 64 or not), every other block flagged
template <typename T>
static void run_adam(long n, int decoupled, double tol) {
  const long nb = (n + 63) / 64;
  std::vector<uint8_t> table((size_t)nb), none((size_t)nb, 0), all((size_t)nb, 1);
  for (long b = 0; b < nb; ++b) table[b] = (uint8_t)(b & 1);
  std::vector<T> p0((size_t)n), g((size_t)n);
  for (auto& v : p0) v = (T)rnd();
  for (auto& v : g) v = (T)rnd();
  const double lr = 0.01, b1 = 0.9, b2 = 0.999, eps = 1e-8, wd = 0.1;
  auto steps = [&](const uint8_t* t, double w, std::vector<T>& p) {
    p = p0;
    std::vector<T> m((size_t)n, (T)0), v((size_t)n, (T)0);
    for (int s = 1; s <= 3; ++s) {
      const double bc1 = 1 - std::pow(b1, s), bc2 = 1 - std::pow(b2, s);
      if (t) adam_step_nodecay<T>(p.data(), g.data(), m.data(), v.data(), n, lr, b1, b2, eps, bc1, bc2, w, decoupled, t);
      else adam_step<T>(p.data(), g.data(), m.data(), v.data(), n, lr, b1, b2, eps, bc1, bc2, w, decoupled);
    }
  };
  std::vector<T> mixed, plain, nodecay, allflag, noflag;
  steps(table.data(), wd, mixed);
  steps(nullptr, wd, plain);
  steps(nullptr, 0.0, nodecay);
  steps(all.data(), wd, allflag);
  steps(none.data(), wd, noflag);
  for (long i = 0; i < n; ++i) {
    CHECK(allflag[i] == nodecay[i]);  // everything flagged: wd = 0, bit for bit
    CHECK(noflag[i] == plain[i]);     // nothing flagged: adam_step, bit for bit
    CHECK(mixed[i] == (((i >> 6) & 1) ? nodecay[i] : plain[i]));
  }
  // and against the formula in double
  std::vector<double> r((size_t)n), m((size_t)n, 0.0), v((size_t)n, 0.0);
  for (long i = 0; i < n; ++i) r[i] = p0[i];
  for (int s = 1; s <= 3; ++s) {
    const double bc1 = 1 - std::pow(b1, s), bc2 = 1 - std::pow(b2, s);
    for (long i = 0; i < n; ++i) {
      const double w = ((i >> 6) & 1) ? 0.0 : wd, gi = g[i];
      m[i] = b1 * m[i] + (1 - b1) * gi;
      v[i] = b2 * v[i] + (1 - b2) * gi * gi;
      double upd = lr * (m[i] / bc1) / (std::sqrt(v[i] / bc2) + eps);
      if (decoupled) r[i] -= w * lr * r[i];
      else upd += w * lr * r[i];
      r[i] -= upd;
    }
  }
  for (long i = 0; i < n; ++i) CHECK(std::fabs((double)mixed[i] - r[i]) < tol);
}

int main() {
  run_mask();
  const long shapes[][2] = {{1, 1}, {5, 72}, {3, 7}, {4, 16}, {2, 2048}, {64, 3}};
  for (const auto& s : shapes) {
    run_scale<float>(s[0], s[1]);
    run_scale<double>(s[0], s[1]);
  }
  for (long n : {64l, 256l, 200l, 70l, 8192l + 64l})
    for (int dec : {0, 1}) {
      run_adam<float>(n, dec, 1e-5);
      run_adam<double>(n, dec, 1e-12);
    }
  std::printf("droppath selftest OK\n");
  return 0;
}
