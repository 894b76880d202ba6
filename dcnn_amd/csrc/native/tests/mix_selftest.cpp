// Stand-alone self-test of the native Mixup / CutMix and soft-target loss CPU code (cpu_ops.cpp
// mix_plan / mix_batch / loss_fused kind 5), float32 and float64, against naive loops. Built under
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_mix_sanitizers.py: heap buffers sized
// exactly (the batch B * C * H * W, the target B * K), so an index past a row, the box or the target
// is a sanitizer report. Covers the odd batch (middle sample untouched), B = 1, rows that are no
// multiple of 4 and boxes touching every edge. Host code only.
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

static unsigned g_state = 24680u;
static double rnd() {
  g_state = g_state * 1664525u + 1013904223u;
  return ((g_state >> 8) & 0xffff) / 32768.0 - 1.0;
}

static void run_plan() {
  for (uint64_t seed : {0ull, 7ull, ~0ull})
    for (uint64_t step = 1; step <= 400; ++step)
      for (int hw : {1, 5, 64}) {
        const MixPlan a = mix_plan(seed, step, hw, hw + 3, 0.8, 1.0, 0.9, 0.5);
        const MixPlan b = mix_plan(seed, step, hw, hw + 3, 0.8, 1.0, 0.9, 0.5);
        CHECK(a.mode == b.mode && a.lam == b.lam && a.yl == b.yl && a.yh == b.yh && a.xl == b.xl && a.xh == b.xh);
        CHECK(a.mode >= 0 && a.mode <= 2 && a.lam >= 0.0 && a.lam <= 1.0);
        if (a.mode == 0) CHECK(a.lam == 1.0);
        if (a.mode == 2) {
          CHECK(0 <= a.yl && a.yl <= a.yh && a.yh <= hw && 0 <= a.xl && a.xl <= a.xh && a.xh <= hw + 3);
          const long area = (long)(a.yh - a.yl) * (a.xh - a.xl);
          CHECK(a.lam == (area ? 1.0 - (double)area / ((double)hw * (hw + 3)) : 1.0));
        } else {
          CHECK(a.yl == 0 && a.yh == 0 && a.xl == 0 && a.xh == 0);
        }
      }
  for (double alpha : {0.05, 0.2, 1.0, 4.0})  // small alphas take the boost path and many rejections
    for (uint64_t step = 1; step <= 2000; ++step) {
      const MixPlan p = mix_plan(11, step, 8, 8, alpha, 0.0, 1.0, 0.5);
      CHECK(p.mode == 1 && p.lam >= 0.0 && p.lam <= 1.0);
    }
  for (uint64_t step = 1; step <= 100; ++step) CHECK(mix_plan(3, step, 8, 8, 0.8, 1.0, 0.0, 0.5).mode == 0);
  int thrown = 0;
  try { mix_plan(0, 1, 8, 8, -1.0, 1.0, 1.0, 0.5); } catch (const std::invalid_argument&) { ++thrown; }
  try { mix_plan(0, 1, 8, 8, 0.8, 1.0, 1.5, 0.5); } catch (const std::invalid_argument&) { ++thrown; }
  try { mix_plan(0, 1, 0, 8, 0.8, 1.0, 1.0, 0.5); } catch (const std::invalid_argument&) { ++thrown; }
  CHECK(thrown == 3);
}

template <typename T>
static void check_target(const std::vector<float>& t, const std::vector<int64_t>& lab, long B, long K, int mode,
                         double lam) {
  const float lamf = (float)lam;
  for (long i = 0; i < B; ++i) {
    const int64_t a = lab[i], b = lab[B - 1 - i];
    const bool one = mode == 0 || a == b || B - 1 - i == i;
    for (long k = 0; k < K; ++k) {
      float want = 0.f;
      if (one) want = k == a ? 1.0f : 0.f;
      else if (k == a) want = lamf;
      else if (k == b) want = 1.0f - lamf;
      CHECK(t[i * K + k] == want);
    }
  }
}

template <typename T>
static void run_batch() {
  struct Row { long C, H, W; };
  const Row rows[] = {{3, 5, 5}, {1, 28, 28}, {2, 4, 6}, {1, 1, 1}};
  for (const Row& r : rows)
    for (long B : {1l, 2l, 5l, 8l})
      for (long K : {1l, 3l, 10l}) {
        const long row = r.C * r.H * r.W;
        std::vector<T> x0((size_t)(B * row));
        for (T& v : x0) v = (T)rnd();
        std::vector<int64_t> lab((size_t)B);
        for (long i = 0; i < B; ++i) lab[i] = (int64_t)((i * 7 + 1) % (K + 1)) - (i == 3 ? 2 : 0);  // some outside [0, K)
        if (B >= 2) lab[B - 1] = lab[0];
        // mode 0
        {
          std::vector<T> x = x0;
          std::vector<float> t((size_t)(B * K), -7.f);
          mix_batch<T>(x.data(), lab.data(), t.data(), B, r.C, r.H, r.W, 0, 0.3, 0, 0, 0, 0, K);
          CHECK(x == x0);
          check_target<T>(t, lab, B, K, 0, 0.3);
        }
        // Mixup: the kernel's rounding, written out
        for (double lam : {0.0, 0.3, 1.0}) {
          std::vector<T> x = x0;
          std::vector<float> t((size_t)(B * K), -7.f);
          mix_batch<T>(x.data(), lab.data(), t.data(), B, r.C, r.H, r.W, 1, lam, 0, 0, 0, 0, K);
          const T l = (T)lam, o = (T)1 - l;
          for (long i = 0; i < B; ++i) {
            const long j = B - 1 - i;
            for (long e = 0; e < row; ++e) {
              const T a = x0[i * row + e], b = x0[j * row + e];
              const T pb = o * b;
              const T want = i == j ? a : (T)std::fma(l, a, pb);
              CHECK(x[i * row + e] == want);
              CHECK(std::fabs((double)x[i * row + e] - (lam * (double)a + (1.0 - lam) * (double)b)) <=
                    4.0 * std::ldexp(1.0, -24) * (std::fabs((double)a) + std::fabs((double)b)));
            }
          }
          check_target<T>(t, lab, B, K, 1, lam);
        }
        // CutMix: full image, one pixel, each edge, empty
        const int H = (int)r.H, W = (int)r.W;
        const int boxes[][4] = {{0, H, 0, W}, {H / 2, H / 2 + 1, W / 2, W / 2 + 1}, {0, 1, 0, W}, {H - 1, H, 0, W},
                                {0, H, 0, 1}, {0, H, W - 1, W}, {H, H, 0, W}};
        for (const auto& bx : boxes) {
          std::vector<T> x = x0;
          std::vector<float> t((size_t)(B * K), -7.f);
          const double lam = 1.0 - (double)((bx[1] - bx[0]) * (bx[3] - bx[2])) / (double)(H * W);
          mix_batch<T>(x.data(), lab.data(), t.data(), B, r.C, r.H, r.W, 2, lam, bx[0], bx[1], bx[2], bx[3], K);
          for (long i = 0; i < B; ++i)
            for (long c = 0; c < r.C; ++c)
              for (int yy = 0; yy < H; ++yy)
                for (int xx = 0; xx < W; ++xx) {
                  const bool in = yy >= bx[0] && yy < bx[1] && xx >= bx[2] && xx < bx[3];
                  const long o = (c * H + yy) * W + xx;
                  CHECK(x[i * row + o] == x0[(in ? B - 1 - i : i) * row + o]);
                }
          check_target<T>(t, lab, B, K, 2, lam);
        }
      }
  // bad arguments
  std::vector<T> x(2 * 16);
  std::vector<int64_t> lab(2, 0);
  std::vector<float> t(2 * 3);
  int thrown = 0;
  try { mix_batch<T>(x.data(), lab.data(), t.data(), 2, 1, 4, 4, 1, 1.5, 0, 0, 0, 0, 3); } catch (const std::invalid_argument&) { ++thrown; }
  try { mix_batch<T>(x.data(), lab.data(), t.data(), 2, 1, 4, 4, 2, 0.5, 0, 5, 0, 4, 3); } catch (const std::invalid_argument&) { ++thrown; }
  try { mix_batch<T>(x.data(), lab.data(), t.data(), 2, 1, 4, 4, 2, 0.5, 0, 4, -1, 4, 3); } catch (const std::invalid_argument&) { ++thrown; }
  try { mix_batch<T>(x.data(), lab.data(), t.data(), 2, 1, 4, 4, 1, 0.5, 0, 0, 0, 0, 0); } catch (const std::invalid_argument&) { ++thrown; }
  try { mix_batch<T>(x.data(), lab.data(), t.data(), 2, 1, 4, 4, 3, 0.5, 0, 0, 0, 0, 3); } catch (const std::invalid_argument&) { ++thrown; }
  CHECK(thrown == 5);
}

template <typename T>
static void run_loss(double tol) {
  for (long N : {1l, 5l, 33l})
    for (long C : {1l, 3l, 10l, 200l})
      for (double eps : {0.0, 0.1})
        for (int dense = 0; dense < 2; ++dense) {
          std::vector<T> p((size_t)(N * C)), t((size_t)(N * C), (T)0), g((size_t)(N * C), (T)-9);
          std::vector<int64_t> lab((size_t)N);
          for (T& v : p) v = (T)(3.0 * rnd());
          for (long n = 0; n < N; ++n) {
            lab[n] = (n * 5 + 2) % C;
            const double lam = 0.5 + 0.5 * rnd();
            t[n * C + lab[n]] += (T)lam;
            t[n * C + (n * 3) % C] += (T)(1.0 - lam);
          }
          long correct = -1;
          const double loss = loss_fused<T>(5, p.data(), dense ? t.data() : nullptr, lab.data(), g.data(), N, C, eps,
                                            &correct);
          double want = 0.0;
          long hits = 0;
          for (long n = 0; n < N; ++n) {
            auto tg = [&](long c) { return dense ? (double)t[n * C + c] : (double)(lab[n] == c); };
            double m = p[n * C];
            for (long c = 1; c < C; ++c) m = std::max(m, (double)p[n * C + c]);
            double z = 0.0;
            for (long c = 0; c < C; ++c) z += std::exp((double)p[n * C + c] - m);
            const double lse = m + std::log(z);
            double S = 0.0, dot = 0.0;
            for (long c = 0; c < C; ++c) {
              const double ts = (1.0 - eps) * tg(c) + eps / (double)C;
              S += ts;
              dot += ts * (double)p[n * C + c];
            }
            want += S * lse - dot;
            long am = 0, tam = 0;
            for (long c = 1; c < C; ++c) {
              if (p[n * C + c] > p[n * C + am]) am = c;
              if (tg(c) > tg(tam)) tam = c;
            }
            hits += am == tam;
            for (long c = 0; c < C; ++c) {
              const double ts = (1.0 - eps) * tg(c) + eps / (double)C;
              const double gw = (S * std::exp((double)p[n * C + c] - lse) - ts) / (double)N;
              CHECK(std::fabs((double)g[n * C + c] - gw) <= tol * std::fabs(gw) + 1e-7);
            }
          }
          want /= (double)N;
          CHECK(std::fabs(loss - want) <= 1e-12 * std::max(1.0, std::fabs(want)));
          CHECK(correct == hits);
          // no gradient wanted: the value alone
          CHECK(loss_fused<T>(5, p.data(), dense ? t.data() : nullptr, lab.data(), nullptr, N, C, eps, nullptr) == loss);
        }
  int thrown = 0;
  std::vector<T> p(3, (T)0), g(3);
  std::vector<int64_t> lab(1, 0);
  try { loss_fused<T>(5, p.data(), nullptr, lab.data(), g.data(), 1, 3, 1.0, nullptr); } catch (const std::invalid_argument&) { ++thrown; }
  try { loss_fused<T>(5, p.data(), nullptr, lab.data(), g.data(), 1, 3, -0.5, nullptr); } catch (const std::invalid_argument&) { ++thrown; }
  try { loss_fused<T>(6, p.data(), nullptr, lab.data(), g.data(), 1, 3, 0.0, nullptr); } catch (const std::invalid_argument&) { ++thrown; }
  CHECK(thrown == 3);
}

int main() {
  run_plan();
  run_batch<float>();
  run_batch<double>();
  run_loss<float>(1e-5);
  run_loss<double>(1e-12);
  std::printf("mix selftest OK\n");
  return 0;
}
