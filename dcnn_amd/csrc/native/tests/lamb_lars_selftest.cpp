// Stand-alone self-test of the layer-wise optimizers' CPU code: the segment / chunk table builder
// (csrc/kernels/optim_segments.cpp) and the native steps (cpu_ops.cpp lamb_step / lars_step), float32
// and float64, against naive per-parameter loops. Built under AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_lamb_lars_sanitizers.py: heap buffers sized exactly (the
// padded arena, the tables row for row, 3 doubles per segment), so an index past a buffer or a table is a
// sanitizer report. Covers tiny and ragged slices, an empty parameter list, a lone unpadded parameter
// (the chunk cut at n), flagged parameters, and every optional input absent. Host code only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "../../kernels/optim_segments.h"
#include "../cpu_kernels.h"

using namespace dcnn_native::cpu;
using dcnn::OptimSegments;

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

static bool close(double a, double b, double tol) { return std::fabs(a - b) <= tol * (1.0 + std::fabs(b)); }

struct Arena {
  std::vector<long> off, cnt;
  std::vector<unsigned char> flag;
  long n = 0;
  std::vector<int> chunks, segs;
};

static Arena make(const std::vector<long>& counts, bool exclude) {
  Arena a;
  for (size_t i = 0; i < counts.size(); ++i) {
    a.off.push_back(a.n);
    a.cnt.push_back(counts[i]);
    a.flag.push_back((unsigned char)(i % 3 == 1));
    a.n += (counts[i] + 63) / 64 * 64;
  }
  const OptimSegments t = dcnn::build_optim_segments(a.off.data(), a.cnt.data(), a.flag.data(), (int)counts.size(),
                                                     exclude, a.n);
  dcnn::check_optim_segments(t.chunks.data(), (int)t.chunks.size(), t.segs.data(), (int)t.segs.size(), a.n);
  CHECK(t.cover == a.n && t.segs.size() == counts.size());
  // the chunks tile the arena exactly, none straddles a slice, each segment's rows are contiguous
  std::vector<int> seen((size_t)(a.n / 64), 0);
  size_t row = 0;
  for (size_t s = 0; s < counts.size(); ++s) {
    CHECK(t.segs[s].first_chunk == (int)row && t.segs[s].chunks == (int)((counts[s] + 4095) / 4096));
    CHECK(t.segs[s].adapt == ((exclude && a.flag[s]) ? 0 : 1) && t.segs[s].decay == t.segs[s].adapt);
    for (int k = 0; k < t.segs[s].chunks; ++k, ++row) {
      const dcnn::SegChunk& c = t.chunks[row];
      CHECK(c.segment == (int)s && c.blocks >= 1 && c.blocks <= 64);
      CHECK((long)c.first_block * 64 >= a.off[s] && ((long)c.first_block + c.blocks) * 64 <= a.off[s] + (a.cnt[s] + 63) / 64 * 64);
      for (int b = 0; b < c.blocks; ++b) ++seen[(size_t)c.first_block + b];
    }
  }
  CHECK(row == t.chunks.size());
  for (int v : seen) CHECK(v == 1);
  for (const auto& c : t.chunks) a.chunks.insert(a.chunks.end(), {c.first_block, c.blocks, c.segment});
  for (const auto& g : t.segs) a.segs.insert(a.segs.end(), {g.first_chunk, g.chunks, g.adapt, g.decay});
  return a;
}

template <typename T>
static std::vector<T> fill(const Arena& a, double scale) {
  std::vector<T> v((size_t)a.n, (T)0);  // zero in the gaps
  for (size_t s = 0; s < a.cnt.size(); ++s)
    for (long i = 0; i < a.cnt[s]; ++i) v[(size_t)(a.off[s] + i)] = (T)(rnd() * scale);
  return v;
}

template <typename T>
static void run(const std::vector<long>& counts, bool lamb, bool exclude, bool with_coef, bool with_ema, bool momentum,
                double tol) {
  const double lr = 0.01, b1 = 0.9, b2 = 0.999, eps = 1e-6, bc1 = 0.19, bc2 = 0.002, wd = 0.1, decay = 0.9, coef = 0.3;
  const double mom = momentum ? 0.9 : 0.0, tc = 0.02, leps = 1e-8;
  const Arena a = make(counts, exclude);
  std::vector<T> p = fill<T>(a, 1.0), g = fill<T>(a, 2.0), m = fill<T>(a, 0.1), v = fill<T>(a, 0.3);
  for (auto& x : v) x = x * x;
  std::vector<T> ema = p;
  const std::vector<T> p0 = p, m0 = m, v0 = v, e0 = ema;
  std::vector<double> out(3 * counts.size(), -1.0);
  const double c = with_coef ? coef : 1.0;
  if (lamb)
    lamb_step<T>(p.data(), g.data(), m.data(), v.data(), a.n, lr, b1, b2, eps, bc1, bc2, wd, with_coef ? &coef : nullptr,
                 with_ema ? ema.data() : nullptr, decay, a.chunks.data(), (int)a.chunks.size() / 3, a.segs.data(),
                 (int)counts.size(), out.data());
  else
    lars_step<T>(p.data(), g.data(), momentum ? m.data() : nullptr, a.n, lr, mom, wd, tc, leps,
                 with_coef ? &coef : nullptr, with_ema ? ema.data() : nullptr, decay, a.chunks.data(),
                 (int)a.chunks.size() / 3, a.segs.data(), (int)counts.size(), out.data());
  for (size_t s = 0; s < counts.size(); ++s) {
    const bool flagged = exclude && a.flag[s];
    const double w = flagged ? 0.0 : wd;
    const long o = a.off[s], n = a.cnt[s];
    std::vector<double> u((size_t)n), mm((size_t)n), vv((size_t)n);
    double sp = 0.0, su = 0.0;
    for (long i = 0; i < n; ++i) {
      const double pi = p0[(size_t)(o + i)], gi = (double)g[(size_t)(o + i)] * c;
      sp += pi * pi;
      if (lamb) {
        mm[(size_t)i] = (double)(T)(b1 * m0[(size_t)(o + i)] + (1 - b1) * gi);
        vv[(size_t)i] = (double)(T)(b2 * v0[(size_t)(o + i)] + (1 - b2) * gi * gi);
        u[(size_t)i] = (mm[(size_t)i] / bc1) / (std::sqrt(vv[(size_t)i] / bc2) + eps) + w * pi;
        su += u[(size_t)i] * u[(size_t)i];
      } else {
        u[(size_t)i] = gi + w * pi;
        su += (double)g[(size_t)(o + i)] * (double)g[(size_t)(o + i)];
      }
    }
    double trust = 1.0;
    const double pn = std::sqrt(sp), un = lamb ? std::sqrt(su) : c * std::sqrt(su);
    if (!flagged && pn != 0.0 && un != 0.0) trust = lamb ? pn / un : tc * pn / (un + w * pn + leps);
    CHECK(close(out[s], trust, tol));
    CHECK(close(out[counts.size() + 2 * s], sp, tol) && close(out[counts.size() + 2 * s + 1], su, tol));
    if (flagged) CHECK(out[s] == 1.0);
    for (long i = 0; i < n; ++i) {
      const size_t k = (size_t)(o + i);
      double want;
      if (lamb) {
        CHECK(close(m[k], mm[(size_t)i], tol) && close(v[k], vv[(size_t)i], tol));
        want = p0[k] - lr * trust * u[(size_t)i];
      } else if (momentum) {
        const double vel = mom * m0[k] - lr * trust * u[(size_t)i];
        CHECK(close(m[k], vel, tol));
        want = p0[k] + vel;
      } else {
        CHECK(m[k] == m0[k]);
        want = p0[k] - lr * trust * u[(size_t)i];
      }
      CHECK(close(p[k], want, tol));
      if (with_ema) CHECK(close(ema[k], decay * e0[k] + (1 - decay) * want, tol));
      else CHECK(ema[k] == e0[k]);
    }
    for (long i = n; i < (n + 63) / 64 * 64; ++i) CHECK(p[(size_t)(o + i)] == (T)0);  // the gap stays zero
  }
}

// one unpadded parameter of n elements as a single segment of a table for the padded size: the steps
// cut the last chunk at n (the C++ front end's per-parameter CPU path)
template <typename T>
static void run_lone(long n) {
  const long off = 0;
  const OptimSegments t = dcnn::build_optim_segments(&off, &n, nullptr, 1, false, (n + 63) / 64 * 64);
  std::vector<int> chunks, segs;
  for (const auto& c : t.chunks) chunks.insert(chunks.end(), {c.first_block, c.blocks, c.segment});
  for (const auto& g : t.segs) segs.insert(segs.end(), {g.first_chunk, g.chunks, g.adapt, g.decay});
  std::vector<T> p((size_t)n), g((size_t)n), m((size_t)n, (T)0), v((size_t)n, (T)0);
  for (long i = 0; i < n; ++i) {
    p[(size_t)i] = (T)rnd();
    g[(size_t)i] = (T)rnd();
  }
  double out[3];
  lamb_step<T>(p.data(), g.data(), m.data(), v.data(), n, 0.01, 0.9, 0.999, 1e-6, 0.1, 0.001, 0.1, nullptr, nullptr, 0.0,
               chunks.data(), (int)chunks.size() / 3, segs.data(), 1, out);
  CHECK(std::isfinite(out[0]) && out[0] > 0.0);
  lars_step<T>(p.data(), g.data(), nullptr, n, 0.1, 0.0, 0.1, 0.02, 1e-8, nullptr, nullptr, 0.0, chunks.data(),
               (int)chunks.size() / 3, segs.data(), 1, out);
  CHECK(std::isfinite(out[0]) && out[0] > 0.0);
}

static void builder_errors() {
  auto throws = [](const std::vector<long>& off, const std::vector<long>& cnt, long n) {
    try {
      dcnn::build_optim_segments(off.data(), cnt.data(), nullptr, (int)off.size(), false, n);
    } catch (const std::invalid_argument&) {
      return true;
    }
    return false;
  };
  CHECK(throws({0, 70}, {70, 8}, 256));    // not 64-element aligned
  CHECK(throws({0, 64}, {70, 8}, 256));    // overlaps its predecessor
  CHECK(throws({0, 128}, {70, 8}, 128));   // ends past the arena
  CHECK(!throws({0, 128}, {70, 8}, 192));
  const OptimSegments none = dcnn::build_optim_segments(nullptr, nullptr, nullptr, 0, false, 64);
  CHECK(none.chunks.empty() && none.segs.empty() && none.cover == 0);
  const dcnn::SegChunk bad = {0, 65, 0};
  const dcnn::SegInfo seg = {0, 1, 1, 1};
  bool caught = false;
  try {
    dcnn::check_optim_segments(&bad, 1, &seg, 1, 1 << 20);
  } catch (const std::invalid_argument&) {
    caught = true;
  }
  CHECK(caught);
}

int main() {
  const std::vector<std::vector<long>> arenas = {
      {1}, {64}, {1, 63, 64, 65, 4096, 4097, 3 * 4096 + 5}, {5, 0, 7}, std::vector<long>(70, 3)};
  for (const auto& counts : arenas)
    for (int lamb = 0; lamb < 2; ++lamb)
      for (int exclude = 0; exclude < 2; ++exclude)
        for (int opt = 0; opt < 4; ++opt)
          for (int mom = 0; mom < (lamb ? 1 : 2); ++mom) {
            run<float>(counts, lamb != 0, exclude != 0, (opt & 1) != 0, (opt & 2) != 0, mom != 0, 2e-5);
            run<double>(counts, lamb != 0, exclude != 0, (opt & 1) != 0, (opt & 2) != 0, mom != 0, 1e-12);
          }
  {
    Arena empty = make({}, false);
    double none = 0.0;
    float z = 0.f;
    lamb_step<float>(&z, &z, &z, &z, 0, 0.01, 0.9, 0.999, 1e-6, 0.1, 0.001, 0.1, nullptr, nullptr, 0.0, nullptr, 0,
                     nullptr, 0, &none);
    CHECK(empty.chunks.empty() && none == 0.0);
  }
  for (long n : {1L, 63L, 65L, 4097L}) {
    run_lone<float>(n);
    run_lone<double>(n);
  }
  builder_errors();
  std::printf("lamb lars selftest OK\n");
  return 0;
}
