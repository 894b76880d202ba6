// Stand-alone self-test of the native gradient-clipping / weight-EMA CPU kernels (cpu_ops.cpp
// grad_sumsq / adam_step_tail / sgd_step_tail / ema_swap), float32 and float64, against naive loops.
// Built under AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_optim_tail_sanitizers.py:
// heap buffers sized exactly (n elements, the block table one byte per 64 elements), so an index past a
// buffer or the table is a sanitizer report. Covers n = 1, ragged n, n above one thread-pool chunk, and
// every optional input absent (a null nodecay table, a null coefficient, a null EMA buffer). Host code only.
#include <cmath>
#include <cstdint>
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

static unsigned g_state = 24680u;
static double rnd() {
  g_state = g_state * 1664525u + 1013904223u;
  return ((g_state >> 8) & 0xffff) / 32768.0 - 1.0;
}

template <typename T>
static std::vector<T> fill(long n, double scale) {
  std::vector<T> v((size_t)n);
  for (auto& x : v) x = (T)(rnd() * scale);
  return v;
}

template <typename T>
static bool close(T a, double b, double tol) {
  return std::fabs((double)a - b) <= tol * (1.0 + std::fabs(b));
}

template <typename T>
static void run_sumsq(long n, double tol) {
  const std::vector<T> g = fill<T>(n, 3.0);
  double want = 0.0;
  for (T x : g) want += (double)x * (double)x;
  const double got = grad_sumsq<T>(g.data(), n);
  CHECK(std::fabs(got - want) <= tol * want + 1e-300);
  CHECK(grad_sumsq<T>(g.data(), n) == got);  // a fixed order: the same bits again
  const std::vector<T> z((size_t)n, (T)0);
  CHECK(grad_sumsq<T>(z.data(), n) == 0.0);
}

template <typename T>
static void run_adam(long n, int decoupled, bool with_table, bool with_coef, bool with_ema, double tol) {
  const double lr = 0.01, b1 = 0.9, b2 = 0.999, eps = 1e-8, wd = 0.1, decay = 0.9, coef = 0.3;
  std::vector<uint8_t> table((size_t)((n + 63) / 64));
  for (size_t b = 0; b < table.size(); ++b) table[b] = (uint8_t)(b & 1);
  std::vector<T> p = fill<T>(n, 1.0), m((size_t)n, (T)0), v((size_t)n, (T)0), ema = p;
  std::vector<double> rp(p.begin(), p.end()), rm((size_t)n, 0.0), rv((size_t)n, 0.0), re(p.begin(), p.end());
  for (int t = 1; t <= 3; ++t) {
    const std::vector<T> g = fill<T>(n, t == 2 ? 100.0 : 1.0);
    const double bc1 = 1.0 - std::pow(b1, t), bc2 = 1.0 - std::pow(b2, t);
    adam_step_tail<T>(p.data(), g.data(), m.data(), v.data(), n, lr, b1, b2, eps, bc1, bc2, wd, decoupled,
                      with_table ? table.data() : nullptr, with_coef ? &coef : nullptr,
                      with_ema ? ema.data() : nullptr, decay);
    for (long i = 0; i < n; ++i) {
      const double gi = (double)g[i] * (with_coef ? coef : 1.0);
      const double w = with_table && table[(size_t)(i >> 6)] ? 0.0 : wd;
      rm[i] = b1 * rm[i] + (1.0 - b1) * gi;
      rv[i] = b2 * rv[i] + (1.0 - b2) * gi * gi;
      double upd = lr * (rm[i] / bc1) / (std::sqrt(rv[i] / bc2) + eps);
      if (decoupled) rp[i] -= w * lr * rp[i];
      else upd += w * lr * rp[i];
      rp[i] -= upd;
      re[i] = decay * re[i] + (1.0 - decay) * rp[i];
    }
  }
  for (long i = 0; i < n; ++i) {
    CHECK(close(p[i], rp[i], tol));
    if (with_ema) CHECK(close(ema[i], re[i], tol));
  }
  if (!with_table && !with_coef && !with_ema) {  // nothing on: adam_step, bit for bit
    g_state = 1357u;
    std::vector<T> q = fill<T>(n, 1.0), q2 = q, m1((size_t)n, (T)0), v1((size_t)n, (T)0), m2 = m1, v2 = v1;
    const std::vector<T> g = fill<T>(n, 1.0);
    adam_step<T>(q.data(), g.data(), m1.data(), v1.data(), n, lr, b1, b2, eps, 0.1, 0.001, wd, decoupled);
    adam_step_tail<T>(q2.data(), g.data(), m2.data(), v2.data(), n, lr, b1, b2, eps, 0.1, 0.001, wd, decoupled,
                      nullptr, nullptr, nullptr, 0.0);
    CHECK(q == q2 && m1 == m2 && v1 == v2);
    const double one = 1.0;  // and a coefficient of exactly 1 changes no bit
    std::vector<T> q3 = q2, m3 = m2, v3 = v2;
    adam_step<T>(q.data(), g.data(), m1.data(), v1.data(), n, lr, b1, b2, eps, 0.19, 0.002, wd, decoupled);
    adam_step_tail<T>(q3.data(), g.data(), m3.data(), v3.data(), n, lr, b1, b2, eps, 0.19, 0.002, wd, decoupled,
                      nullptr, &one, nullptr, 0.0);
    CHECK(q == q3 && m1 == m3 && v1 == v3);
  }
}

template <typename T>
static void run_sgd(long n, bool momentum, bool with_coef, bool with_ema, double tol) {
  const double lr = 0.05, mom = 0.9, decay = 0.9, coef = 0.25;
  std::vector<T> p = fill<T>(n, 1.0), vel((size_t)n, (T)0), ema = p;
  std::vector<double> rp(p.begin(), p.end()), rv((size_t)n, 0.0), re(p.begin(), p.end());
  for (int t = 1; t <= 3; ++t) {
    const std::vector<T> g = fill<T>(n, 1.0);
    sgd_step_tail<T>(p.data(), g.data(), momentum ? vel.data() : nullptr, n, lr, mom, with_coef ? &coef : nullptr,
                     with_ema ? ema.data() : nullptr, decay);
    for (long i = 0; i < n; ++i) {
      const double gi = (double)g[i] * (with_coef ? coef : 1.0);
      if (momentum) {
        rv[i] = mom * rv[i] - lr * gi;
        rp[i] += rv[i];
      } else {
        rp[i] -= lr * gi;
      }
      re[i] = decay * re[i] + (1.0 - decay) * rp[i];
    }
  }
  for (long i = 0; i < n; ++i) {
    CHECK(close(p[i], rp[i], tol));
    if (with_ema) CHECK(close(ema[i], re[i], tol));
  }
}

template <typename T>
static void run_swap(long n) {
  std::vector<T> a = fill<T>(n, 1.0), b = fill<T>(n, 1.0);
  const std::vector<T> a0 = a, b0 = b;
  ema_swap<T>(a.data(), b.data(), n);
  CHECK(a == b0 && b == a0);
  ema_swap<T>(a.data(), b.data(), n);
  CHECK(a == a0 && b == b0);
}

int main() {
  for (long n : {1l, 3l, 63l, 64l, 65l, 130l, 4099l, 40000l}) {
    run_sumsq<float>(n, 1e-6);
    run_sumsq<double>(n, 1e-13);
    run_swap<float>(n);
    run_swap<double>(n);
    for (int mask = 0; mask < 8; ++mask) {
      const bool tab = mask & 1, cf = mask & 2, em = mask & 4;
      for (int dec = 0; dec < 2; ++dec) {
        run_adam<float>(n, dec, tab, cf, em, 2e-5);
        run_adam<double>(n, dec, tab, cf, em, 1e-12);
      }
      if (!tab)
        for (int momentum = 0; momentum < 2; ++momentum) {
          run_sgd<float>(n, momentum, cf, em, 2e-6);
          run_sgd<double>(n, momentum, cf, em, 1e-13);
        }
    }
  }
  std::printf("optim tail selftest OK\n");
  return 0;
}
