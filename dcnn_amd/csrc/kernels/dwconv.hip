// Depthwise convolution (groups = C, channel multiplier 1) on NHWC activations: forward, data
// gradient (gather form) and weight gradient (slab per split, reduced by splitk_reduce*).
//
// No reduction over channels and KH*KW MACs per element: these are bandwidth-bound streaming
// kernels, not GEMMs. A lane owns one 16-byte channel vector (8 bf16 / 4 fp32 channels); every
// global access is that vector. A workgroup of 256 lanes is laid out channel-vector fastest
// (cvb = min(C / VEC, 64) vectors, C / VEC need not be a power of two), then PB = 256 / cvb work
// items along x, so one wave instruction touches runs of contiguous NHWC bytes.
//
// Compile-time instances (3x3, pad 1, stride 1 or 2 — all of MobileNet): the lane's 9 x VEC
// weights sit in registers as fp32, loaded once per lane (grid-stride loop at a fixed channel
// vector); each work item is a run of kRun = 4 outputs along x computed from a register window of
// input vectors, row by row (stride 1: 3 x 6 loads for 4 outputs instead of 36; the overlap
// between neighbouring lanes / rows is left to L1 / L2 — no LDS halo staging).
// Run-time instance (everything else dwconv_supported admits): one output per work item, the
// workgroup's weights in LDS ([tap][vector][VEC] fp32, cvb <= 16: 25 KB at 49 taps) — a
// dynamically indexed register array would go to scratch. Its weight gradient handles the taps in
// groups of 9 (grid.z), so the accumulators stay in registers.
//
// Weight gradient: a lane accumulates KH*KW x VEC (+ VEC bias) fp32 partials over its share of the
// split's work items; the PB lanes of a workgroup sharing a channel vector are summed in a fixed
// order (wave butterfly, then the wave sums through LDS) and one slab row is written per
// workgroup. The split -> item range mapping is a pure function of the shape, no float atomics
// anywhere: two runs give the same bits.
#include "api.h"
#include "common.h"

namespace dcnn {
namespace {

constexpr int kDwThreads = 256;
constexpr int kRun = 4;        // outputs along x per work item (compile-time instances)
constexpr int kCvbFast = 64;   // channel vectors per workgroup, compile-time instances
constexpr int kCvbRt = 16;     // run-time instance (bounds the LDS weight tile)
constexpr int kMaxTaps = 49;
constexpr int kTapGroup = 9;   // taps per pass of the run-time weight gradient
// Grid sizing. Forward / dgrad: at most kDwGridCap workgroups — 3 per CU, what the compile-time
// bf16 instances' ~160 VGPRs keep resident, so the grid-stride loop runs as one round without a
// tail and a lane amortises its weight loads over several work items at the large maps.
// (Measured alternative, profiles/dwconv.md: branch-free clamped loads + selects put the whole
// window's 18 / 27 loads in flight per wave at 2 waves per SIMD and were no faster.)
// Weight gradient (dw_wgrad_geom): splits = min(output pixels / kDwMinSplitPixels, kDwWgradGrid /
// (channel chunks x tap groups)), at least 1: every split streams >= 512 output pixels per channel
// vector, so the slab row it writes and the reduce reads (72 B per channel) stays a few percent of
// the 4 B per pixel and channel it reads. Where that leaves the grid short of 2 workgroups per CU
// (the small, wide maps) the channel chunk per workgroup is halved down to 8 vectors (128
// contiguous bytes per pixel) — more workgroups over the same slab bytes.
constexpr int kDwGridCap = 768;
constexpr int kDwWgradGrid = 512;
constexpr int kDwMinSplitPixels = 512;

template <typename T> struct DwVec;
template <> struct DwVec<bf16> {
  static constexpr int N = 8;
  typedef uint4 Raw;
  static __device__ __forceinline__ Raw zero() { return make_uint4(0, 0, 0, 0); }
  static __device__ __forceinline__ Raw ld(const bf16* p) { return *reinterpret_cast<const uint4*>(p); }
  static __device__ __forceinline__ void cvt(const Raw& r, float* f) { unpack8(r, f); }
  static __device__ __forceinline__ void st(bf16* p, const float* f) { *reinterpret_cast<uint4*>(p) = pack8(f); }
};
template <> struct DwVec<float> {
  static constexpr int N = 4;
  typedef float4 Raw;
  static __device__ __forceinline__ Raw zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ Raw ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ void cvt(const Raw& r, float* f) { f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w; }
  static __device__ __forceinline__ void st(float* p, const float* f) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  }
};

// launch geometry shared by the kernels: work items are (n, row, xr), xr fastest
struct DwK {
  DwArgs g;
  int CV, cvb, PB;      // channel vectors, vectors per workgroup, items per workgroup pass
  int XR, ROWS;         // items per row, rows per image (of the tensor the kernel produces / walks)
  unsigned NR;          // N * ROWS * XR
  unsigned per_split;   // wgrad: items per split
  int w_vec;            // the weight base is 16-byte aligned (a lane's 9 x VEC weights: 9 vector loads)
  int pow2;             // cvb divides 64: lanes sharing a channel vector sit cvb apart in a wave
  FastDiv fxr, frow;
};

struct DwLane {
  int cvl, pl, cv, c0;
  bool active;
};
template <int V>
__device__ __forceinline__ DwLane dw_lane(const DwK& k) {
  DwLane l;
  l.pl = threadIdx.x / k.cvb;
  l.cvl = threadIdx.x - l.pl * k.cvb;
  l.cv = blockIdx.y * k.cvb + l.cvl;
  l.c0 = l.cv * V;
  l.active = l.pl < k.PB && l.cv < k.CV;
  return l;
}
__device__ __forceinline__ void dw_item(const DwK& k, unsigned item, int& n, int& row, int& xr) {
  const unsigned t = fdiv(item, k.fxr);
  xr = (int)(item - t * (unsigned)k.XR);
  const unsigned nn = fdiv(t, k.frow);
  row = (int)(t - nn * (unsigned)k.ROWS);
  n = (int)nn;
}
// the lane's 9 x V weights (w[(c0 + i) * 9 + t], 144 contiguous bytes) as fp32 registers
template <typename T, int V>
__device__ __forceinline__ void dw_load_w9(const T* w, int c0, bool vec, float (*wr)[V]) {
  typedef DwVec<T> VT;
  if (vec) {
    float f[9][V];
#pragma unroll
    for (int r = 0; r < 9; ++r) VT::cvt(VT::ld(w + (size_t)c0 * 9 + r * V), f[r]);
#pragma unroll
    for (int i = 0; i < V; ++i)
#pragma unroll
      for (int t = 0; t < 9; ++t) wr[t][i] = f[(i * 9 + t) / V][(i * 9 + t) % V];
    return;
  }
#pragma unroll
  for (int i = 0; i < V; ++i)
#pragma unroll
    for (int t = 0; t < 9; ++t) wr[t][i] = to_f(w[(size_t)(c0 + i) * 9 + t]);
}

// ---- compile-time 3x3 / pad 1 / stride S ------------------------------------------------------
template <typename T, int S>
__global__ __launch_bounds__(kDwThreads) void dw_fwd3_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                             const float* __restrict__ bias, T* __restrict__ y, DwK k) {
  typedef DwVec<T> VT;
  constexpr int V = VT::N, WIN = (kRun - 1) * S + 3;
  const DwLane l = dw_lane<V>(k);
  if (!l.active) return;
  const int H = k.g.H, W = k.g.W, C = k.g.C, OH = k.g.OH, OW = k.g.OW;
  float wr[9][V];
  dw_load_w9<T, V>(w, l.c0, k.w_vec != 0, wr);
  float b[V];
#pragma unroll
  for (int i = 0; i < V; ++i) b[i] = bias ? bias[l.c0 + i] : 0.f;
  for (unsigned item = blockIdx.x * k.PB + l.pl; item < k.NR; item += gridDim.x * k.PB) {
    int n, oy, xr;
    dw_item(k, item, n, oy, xr);
    const int ox0 = xr * kRun, ix0 = ox0 * S - 1;
    float acc[kRun][V];
#pragma unroll
    for (int j = 0; j < kRun; ++j)
#pragma unroll
      for (int i = 0; i < V; ++i) acc[j][i] = b[i];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * S + ky - 1;
      if ((unsigned)iy >= (unsigned)H) continue;
      const T* row = x + ((size_t)(n * H + iy) * W) * C + l.c0;
      typename VT::Raw win[WIN];
#pragma unroll
      for (int i = 0; i < WIN; ++i) {
        const int ix = ix0 + i;
        win[i] = (unsigned)ix < (unsigned)W ? VT::ld(row + (size_t)ix * C) : VT::zero();
      }
#pragma unroll
      for (int i = 0; i < WIN; ++i) {
        float f[V];
        VT::cvt(win[i], f);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          if (i - kx < 0 || (i - kx) % S != 0 || (i - kx) / S >= kRun) continue;
          const int j = (i - kx) / S;
#pragma unroll
          for (int e = 0; e < V; ++e) acc[j][e] = fmaf(f[e], wr[ky * 3 + kx][e], acc[j][e]);
        }
      }
    }
    T* out = y + ((size_t)(n * OH + oy) * OW) * C + l.c0;
#pragma unroll
    for (int j = 0; j < kRun; ++j)
      if (ox0 + j < OW) VT::st(out + (size_t)(ox0 + j) * C, acc[j]);
  }
}

// dx run [ix0, ix0 + kRun) of row iy: tap (ky, kx) reads dy[(iy + 1 - ky) / S][(ix + 1 - kx) / S]
// where both are divisible and in range. ix0 is a multiple of kRun (a multiple of S), so which
// (j, kx) pairs hit which window column is known at compile time.
template <typename T, int S>
__global__ __launch_bounds__(kDwThreads) void dw_dgrad3_kernel(const T* __restrict__ dy, const T* __restrict__ w,
                                                               const T* __restrict__ res, T* __restrict__ dx, DwK k) {
  typedef DwVec<T> VT;
  static_assert(kRun % S == 0, "run start must stay stride-aligned");
  constexpr int V = VT::N;
  constexpr int CMIN = S == 1 ? -1 : 0, CMAX = kRun / S;  // window columns relative to ix0 / S
  constexpr int WIN = CMAX - CMIN + 1;
  const DwLane l = dw_lane<V>(k);
  if (!l.active) return;
  const int H = k.g.H, W = k.g.W, C = k.g.C, OH = k.g.OH, OW = k.g.OW;
  float wr[9][V];
  dw_load_w9<T, V>(w, l.c0, k.w_vec != 0, wr);
  for (unsigned item = blockIdx.x * k.PB + l.pl; item < k.NR; item += gridDim.x * k.PB) {
    int n, iy, xr;
    dw_item(k, item, n, iy, xr);
    const int ix0 = xr * kRun, ob = ix0 / S;
    float acc[kRun][V];
#pragma unroll
    for (int j = 0; j < kRun; ++j)
#pragma unroll
      for (int i = 0; i < V; ++i) acc[j][i] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int t = iy + 1 - ky;
      if (t < 0 || (S > 1 && (t % S) != 0)) continue;
      const int oy = t / S;
      if (oy >= OH) continue;
      const T* row = dy + ((size_t)(n * OH + oy) * OW) * C + l.c0;
      typename VT::Raw win[WIN];
#pragma unroll
      for (int i = 0; i < WIN; ++i) {
        const int ox = ob + CMIN + i;
        win[i] = (unsigned)ox < (unsigned)OW ? VT::ld(row + (size_t)ox * C) : VT::zero();
      }
#pragma unroll
      for (int i = 0; i < WIN; ++i) {
        float f[V];
        VT::cvt(win[i], f);
#pragma unroll
        for (int j = 0; j < kRun; ++j)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            if (j + 1 - kx != S * (i + CMIN)) continue;
#pragma unroll
            for (int e = 0; e < V; ++e) acc[j][e] = fmaf(f[e], wr[ky * 3 + kx][e], acc[j][e]);
          }
      }
    }
    const size_t o = ((size_t)(n * H + iy) * W) * C + l.c0;
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
      if (ix0 + j >= W) continue;
      const size_t oj = o + (size_t)(ix0 + j) * C;
      if (res) {
        float r[V];
        VT::cvt(VT::ld(res + oj), r);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[j][e] += r[e];
      }
      VT::st(dx + oj, acc[j]);
    }
  }
}

// Sum the PB lanes of the workgroup that share a channel vector and write element q of every
// channel: out[c * ostride + q]. Fixed order: where cvb divides 64 an xor butterfly over the
// wave's lanes cvb apart, then the 4 wave sums through LDS in wave order; otherwise all PB lanes
// through LDS in lane order. All 256 threads call it.
template <int V>
__device__ __forceinline__ void dw_block_reduce(const DwK& k, const DwLane& l, const float* v, float* red, float* out,
                                                int ostride, int q) {
  float s[V];
#pragma unroll
  for (int e = 0; e < V; ++e) s[e] = l.active ? v[e] : 0.f;
  int row = l.pl, rows = k.PB;
  bool writer = l.pl < k.PB;
  if (k.pow2) {
    for (int off = k.cvb; off < kWave; off <<= 1)
#pragma unroll
      for (int e = 0; e < V; ++e) s[e] += __shfl_xor(s[e], off, kWave);
    row = threadIdx.x >> 6;
    rows = kDwThreads / kWave;
    writer = (int)(threadIdx.x & 63) < k.cvb;
  }
  __syncthreads();
  if (writer) {
#pragma unroll
    for (int e = 0; e < V; ++e) red[(row * k.cvb + l.cvl) * V + e] = s[e];
  }
  __syncthreads();
  const int cols = k.cvb * V;
  for (int t = threadIdx.x; t < cols; t += kDwThreads) {
    const int c = blockIdx.y * cols + t;
    if (c >= k.g.C) continue;
    float a = 0.f;
    for (int p = 0; p < rows; ++p) a += red[p * cols + t];
    out[(size_t)c * ostride + q] = a;
  }
}

template <typename T, int S>
__global__ __launch_bounds__(kDwThreads) void dw_wgrad3_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                               float* __restrict__ slab, float* __restrict__ bslab,
                                                               DwK k) {
  typedef DwVec<T> VT;
  constexpr int V = VT::N, WIN = (kRun - 1) * S + 3;
  __shared__ float red[kDwThreads * V];
  const DwLane l = dw_lane<V>(k);
  const int H = k.g.H, W = k.g.W, C = k.g.C, OH = k.g.OH, OW = k.g.OW;
  float acc[9][V], bacc[V];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[t][e] = 0.f;
#pragma unroll
  for (int e = 0; e < V; ++e) bacc[e] = 0.f;
  const unsigned first = blockIdx.x * k.per_split;
  const unsigned last = min(first + k.per_split, k.NR);
  if (l.active) {
    for (unsigned item = first + l.pl; item < last; item += k.PB) {
      int n, oy, xr;
      dw_item(k, item, n, oy, xr);
      const int ox0 = xr * kRun, ix0 = ox0 * S - 1;
      const T* drow = dy + ((size_t)(n * OH + oy) * OW) * C + l.c0;
      float g[kRun][V];
#pragma unroll
      for (int j = 0; j < kRun; ++j) {
        VT::cvt(ox0 + j < OW ? VT::ld(drow + (size_t)(ox0 + j) * C) : VT::zero(), g[j]);
#pragma unroll
        for (int e = 0; e < V; ++e) bacc[e] += g[j][e];
      }
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * S + ky - 1;
        if ((unsigned)iy >= (unsigned)H) continue;
        const T* row = x + ((size_t)(n * H + iy) * W) * C + l.c0;
        typename VT::Raw win[WIN];
#pragma unroll
        for (int i = 0; i < WIN; ++i) {
          const int ix = ix0 + i;
          win[i] = (unsigned)ix < (unsigned)W ? VT::ld(row + (size_t)ix * C) : VT::zero();
        }
#pragma unroll
        for (int i = 0; i < WIN; ++i) {
          float f[V];
          VT::cvt(win[i], f);
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            if (i - kx < 0 || (i - kx) % S != 0 || (i - kx) / S >= kRun) continue;
            const int j = (i - kx) / S;
#pragma unroll
            for (int e = 0; e < V; ++e) acc[ky * 3 + kx][e] = fmaf(f[e], g[j][e], acc[ky * 3 + kx][e]);
          }
        }
      }
    }
  }
  float* out = slab + (size_t)blockIdx.x * C * 9;
#pragma unroll
  for (int t = 0; t < 9; ++t) dw_block_reduce<V>(k, l, acc[t], red, out, 9, t);
  if (bslab) dw_block_reduce<V>(k, l, bacc, red, bslab + (size_t)blockIdx.x * C, 1, 0);
}

// ---- run-time taps ---------------------------------------------------------------------------
// the workgroup's weights as fp32 in LDS: wl[(tap * cvb + cvl) * V + e]
template <typename T, int V>
__device__ __forceinline__ void dw_stage_w(const T* w, const DwK& k, float* wl) {
  const int KK = k.g.KH * k.g.KW, cols = k.cvb * V;
  for (int idx = threadIdx.x; idx < KK * cols; idx += kDwThreads) {
    const int tap = idx / cols, r = idx - tap * cols;
    const int c = blockIdx.y * cols + r;
    wl[idx] = c < k.g.C ? to_f(w[(size_t)c * KK + tap]) : 0.f;
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(kDwThreads) void dw_fwd_rt_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                               const float* __restrict__ bias, T* __restrict__ y, DwK k) {
  typedef DwVec<T> VT;
  constexpr int V = VT::N;
  __shared__ float wl[kMaxTaps * kCvbRt * V];
  dw_stage_w<T, V>(w, k, wl);
  const DwLane l = dw_lane<V>(k);
  if (!l.active) return;
  const DwArgs g = k.g;
  float b[V];
#pragma unroll
  for (int i = 0; i < V; ++i) b[i] = bias ? bias[l.c0 + i] : 0.f;
  for (unsigned item = blockIdx.x * k.PB + l.pl; item < k.NR; item += gridDim.x * k.PB) {
    int n, oy, ox;
    dw_item(k, item, n, oy, ox);
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = b[i];
    for (int ky = 0; ky < g.KH; ++ky) {
      const int iy = oy * g.SH + ky - g.PH;
      if ((unsigned)iy >= (unsigned)g.H) continue;
      for (int kx = 0; kx < g.KW; ++kx) {
        const int ix = ox * g.SW + kx - g.PW;
        if ((unsigned)ix >= (unsigned)g.W) continue;
        float f[V];
        VT::cvt(VT::ld(x + ((size_t)(n * g.H + iy) * g.W + ix) * g.C + l.c0), f);
        const float* wt = wl + ((ky * g.KW + kx) * k.cvb + l.cvl) * V;
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = fmaf(f[e], wt[e], acc[e]);
      }
    }
    VT::st(y + ((size_t)(n * g.OH + oy) * g.OW + ox) * g.C + l.c0, acc);
  }
}

template <typename T>
__global__ __launch_bounds__(kDwThreads) void dw_dgrad_rt_kernel(const T* __restrict__ dy, const T* __restrict__ w,
                                                                 const T* __restrict__ res, T* __restrict__ dx, DwK k) {
  typedef DwVec<T> VT;
  constexpr int V = VT::N;
  __shared__ float wl[kMaxTaps * kCvbRt * V];
  dw_stage_w<T, V>(w, k, wl);
  const DwLane l = dw_lane<V>(k);
  if (!l.active) return;
  const DwArgs g = k.g;
  for (unsigned item = blockIdx.x * k.PB + l.pl; item < k.NR; item += gridDim.x * k.PB) {
    int n, iy, ix;
    dw_item(k, item, n, iy, ix);
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    for (int ky = 0; ky < g.KH; ++ky) {
      const int ty = iy + g.PH - ky;
      if (ty < 0 || ty % g.SH != 0) continue;
      const int oy = ty / g.SH;
      if (oy >= g.OH) continue;
      for (int kx = 0; kx < g.KW; ++kx) {
        const int tx = ix + g.PW - kx;
        if (tx < 0 || tx % g.SW != 0) continue;
        const int ox = tx / g.SW;
        if (ox >= g.OW) continue;
        float f[V];
        VT::cvt(VT::ld(dy + ((size_t)(n * g.OH + oy) * g.OW + ox) * g.C + l.c0), f);
        const float* wt = wl + ((ky * g.KW + kx) * k.cvb + l.cvl) * V;
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = fmaf(f[e], wt[e], acc[e]);
      }
    }
    const size_t o = ((size_t)(n * g.H + iy) * g.W + ix) * g.C + l.c0;
    if (res) {
      float r[V];
      VT::cvt(VT::ld(res + o), r);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += r[e];
    }
    VT::st(dx + o, acc);
  }
}

// taps [blockIdx.z * kTapGroup, + kTapGroup) of the split's output pixels
template <typename T>
__global__ __launch_bounds__(kDwThreads) void dw_wgrad_rt_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                 float* __restrict__ slab, float* __restrict__ bslab,
                                                                 DwK k) {
  typedef DwVec<T> VT;
  constexpr int V = VT::N;
  __shared__ float red[kDwThreads * V];
  const DwLane l = dw_lane<V>(k);
  const DwArgs g = k.g;
  const int KK = g.KH * g.KW, tap0 = blockIdx.z * kTapGroup;
  int tky[kTapGroup], tkx[kTapGroup];  // (statically indexed: the tap loops below are unrolled)
#pragma unroll
  for (int t = 0; t < kTapGroup; ++t) {
    const int tap = min(tap0 + t, KK - 1);
    tky[t] = tap / g.KW - g.PH;
    tkx[t] = tap % g.KW - g.PW;
  }
  float acc[kTapGroup][V], bacc[V];
#pragma unroll
  for (int t = 0; t < kTapGroup; ++t)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[t][e] = 0.f;
#pragma unroll
  for (int e = 0; e < V; ++e) bacc[e] = 0.f;
  const unsigned first = blockIdx.x * k.per_split;
  const unsigned last = min(first + k.per_split, k.NR);
  if (l.active) {
    for (unsigned item = first + l.pl; item < last; item += k.PB) {
      int n, oy, ox;
      dw_item(k, item, n, oy, ox);
      float gv[V];
      VT::cvt(VT::ld(dy + ((size_t)(n * g.OH + oy) * g.OW + ox) * g.C + l.c0), gv);
#pragma unroll
      for (int e = 0; e < V; ++e) bacc[e] += gv[e];
#pragma unroll
      for (int t = 0; t < kTapGroup; ++t) {
        const int iy = oy * g.SH + tky[t], ix = ox * g.SW + tkx[t];
        if (tap0 + t >= KK || (unsigned)iy >= (unsigned)g.H || (unsigned)ix >= (unsigned)g.W) continue;
        float f[V];
        VT::cvt(VT::ld(x + ((size_t)(n * g.H + iy) * g.W + ix) * g.C + l.c0), f);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[t][e] = fmaf(f[e], gv[e], acc[t][e]);
      }
    }
  }
  float* out = slab + (size_t)blockIdx.x * g.C * KK;
#pragma unroll
  for (int t = 0; t < kTapGroup; ++t)
    if (tap0 + t < KK) dw_block_reduce<V>(k, l, acc[t], red, out, KK, tap0 + t);
  if (bslab && blockIdx.z == 0) dw_block_reduce<V>(k, l, bacc, red, bslab + (size_t)blockIdx.x * g.C, 1, 0);
}

// ---- host side -------------------------------------------------------------------------------
inline int dw_vec(int dt) { return dt == 1 ? 8 : 4; }
inline int dw_fast_stride(const DwArgs& g) {  // 1 / 2: a compile-time instance, 0: run-time taps
  if (g.KH == 3 && g.KW == 3 && g.PH == 1 && g.PW == 1 && g.SH == g.SW && (g.SH == 1 || g.SH == 2)) return g.SH;
  return 0;
}
void dw_set_cvb(DwK& k, int cvb) {
  k.cvb = cvb;
  k.PB = kDwThreads / cvb;
  k.pow2 = kWave % cvb == 0;
}
// geometry for a kernel walking `rows` x `cols` maps, `run` columns per item
DwK dw_geom(int dt, const DwArgs& g, int rows, int cols, int run, int cvb_max) {
  DwK k{};
  k.g = g;
  k.CV = g.C / dw_vec(dt);
  k.cvb = k.CV < cvb_max ? k.CV : cvb_max;
  dw_set_cvb(k, k.cvb);
  k.XR = (cols + run - 1) / run;
  k.ROWS = rows;
  k.NR = (unsigned)((long)g.N * rows * k.XR);
  k.per_split = k.NR;
  k.fxr = make_fastdiv((unsigned)k.XR);
  k.frow = make_fastdiv((unsigned)rows);
  return k;
}
dim3 dw_grid(const DwK& k) {
  const int gy = (k.CV + k.cvb - 1) / k.cvb;
  long gx = ((long)k.NR + k.PB - 1) / k.PB;
  const long cap = kDwGridCap / gy > 0 ? kDwGridCap / gy : 1;
  if (gx > cap) gx = cap;
  return dim3((unsigned)(gx < 1 ? 1 : gx), (unsigned)gy, 1);
}
void dw_require(int dt, const DwArgs& g, const char* what) {
  if (!dwconv_supported(dt, g))
    throw std::runtime_error(std::string(what) + ": unsupported depthwise conv (dt " + std::to_string(dt) + ", N " +
                             std::to_string(g.N) + ", C " + std::to_string(g.C) + ", " + std::to_string(g.H) + "x" +
                             std::to_string(g.W) + ", kernel " + std::to_string(g.KH) + "x" + std::to_string(g.KW) +
                             ", stride " + std::to_string(g.SH) + "x" + std::to_string(g.SW) + ", pad " +
                             std::to_string(g.PH) + "x" + std::to_string(g.PW) + ")");
}

template <typename T>
void dw_fwd_t(const void* x, const void* w, const float* bias, void* y, int dt, const DwArgs& g, hipStream_t s) {
  const int fs = dw_fast_stride(g);
  DwK k = fs ? dw_geom(dt, g, g.OH, g.OW, kRun, kCvbFast) : dw_geom(dt, g, g.OH, g.OW, 1, kCvbRt);
  const dim3 grid = dw_grid(k);
  const T *xp = (const T*)x, *wp = (const T*)w;
  k.w_vec = ((uintptr_t)w & 15) == 0;
  if (fs == 1) dw_fwd3_kernel<T, 1><<<grid, kDwThreads, 0, s>>>(xp, wp, bias, (T*)y, k);
  else if (fs == 2) dw_fwd3_kernel<T, 2><<<grid, kDwThreads, 0, s>>>(xp, wp, bias, (T*)y, k);
  else dw_fwd_rt_kernel<T><<<grid, kDwThreads, 0, s>>>(xp, wp, bias, (T*)y, k);
}
template <typename T>
void dw_dgrad_t(const void* dy, const void* w, const void* res, void* dx, int dt, const DwArgs& g, hipStream_t s) {
  const int fs = dw_fast_stride(g);
  DwK k = fs ? dw_geom(dt, g, g.H, g.W, kRun, kCvbFast) : dw_geom(dt, g, g.H, g.W, 1, kCvbRt);
  const dim3 grid = dw_grid(k);
  const T *dp = (const T*)dy, *wp = (const T*)w, *rp = (const T*)res;
  k.w_vec = ((uintptr_t)w & 15) == 0;
  if (fs == 1) dw_dgrad3_kernel<T, 1><<<grid, kDwThreads, 0, s>>>(dp, wp, rp, (T*)dx, k);
  else if (fs == 2) dw_dgrad3_kernel<T, 2><<<grid, kDwThreads, 0, s>>>(dp, wp, rp, (T*)dx, k);
  else dw_dgrad_rt_kernel<T><<<grid, kDwThreads, 0, s>>>(dp, wp, rp, (T*)dx, k);
}
inline int dw_tap_groups(const DwArgs& g) {
  return dw_fast_stride(g) ? 1 : (g.KH * g.KW + kTapGroup - 1) / kTapGroup;
}
// split count for channel chunks of cvb vectors (the rule next to kDwWgradGrid)
int dw_wgrad_splits_for(const DwK& k, int cvb) {
  const DwArgs& g = k.g;
  const long chunks = (long)((k.CV + cvb - 1) / cvb) * dw_tap_groups(g);
  long splits = (long)g.N * g.OH * g.OW / kDwMinSplitPixels;
  if (splits > kDwWgradGrid / chunks) splits = kDwWgradGrid / chunks;
  if (splits > (long)k.NR) splits = k.NR;
  return splits < 1 ? 1 : (int)splits;
}
DwK dw_wgrad_geom(int dt, const DwArgs& g) {
  DwK k = dw_fast_stride(g) ? dw_geom(dt, g, g.OH, g.OW, kRun, kCvbFast) : dw_geom(dt, g, g.OH, g.OW, 1, kCvbRt);
  int cvb = k.cvb;
  while (cvb > 8 && cvb % 2 == 0 &&
         (long)dw_wgrad_splits_for(k, cvb) * ((k.CV + cvb - 1) / cvb) * dw_tap_groups(g) < kDwWgradGrid)
    cvb /= 2;
  dw_set_cvb(k, cvb);
  return k;
}
int dw_wgrad_splits_k(const DwK& k) { return dw_wgrad_splits_for(k, k.cvb); }
template <typename T>
void dw_wgrad_t(const void* dy, const void* x, float* slab, float* bslab, int dt, const DwArgs& g, hipStream_t s) {
  DwK k = dw_wgrad_geom(dt, g);
  const int splits = dw_wgrad_splits_k(k);
  k.per_split = (k.NR + splits - 1) / splits;
  const int fs = dw_fast_stride(g);
  const int gy = (k.CV + k.cvb - 1) / k.cvb;
  const int gz = dw_tap_groups(g);
  const dim3 grid(splits, gy, gz);
  const T *dp = (const T*)dy, *xp = (const T*)x;
  if (fs == 1) dw_wgrad3_kernel<T, 1><<<grid, kDwThreads, 0, s>>>(dp, xp, slab, bslab, k);
  else if (fs == 2) dw_wgrad3_kernel<T, 2><<<grid, kDwThreads, 0, s>>>(dp, xp, slab, bslab, k);
  else dw_wgrad_rt_kernel<T><<<grid, kDwThreads, 0, s>>>(dp, xp, slab, bslab, k);
}

}  // namespace

bool dwconv_supported(int dt, DwArgs g) {
  if (dt != 0 && dt != 1) return false;
  if (g.N < 1 || g.C < 1 || g.H < 1 || g.W < 1 || g.KH < 1 || g.KW < 1 || g.SH < 1 || g.SW < 1) return false;
  if (g.C % dw_vec(dt) != 0 || g.KH * g.KW > kMaxTaps) return false;
  if (g.PH < 0 || g.PW < 0 || g.PH >= g.KH || g.PW >= g.KW) return false;
  if (g.H + 2 * g.PH < g.KH || g.W + 2 * g.PW < g.KW) return false;
  if (g.OH != (g.H + 2 * g.PH - g.KH) / g.SH + 1 || g.OW != (g.W + 2 * g.PW - g.KW) / g.SW + 1) return false;
  const long lim = 1L << 31;
  // element offsets (and the work-item count, at most one per element) stay below 2^31
  return (long)g.N * g.H * g.W * g.C < lim && (long)g.N * g.OH * g.OW * g.C < lim;
}

void dwconv_fwd(int dt, const void* x, const void* w, const float* bias, void* y, DwArgs g, hipStream_t s) {
  dw_require(dt, g, "dwconv_fwd");
  if (dt == 1) dw_fwd_t<bf16>(x, w, bias, y, dt, g, s);
  else dw_fwd_t<float>(x, w, bias, y, dt, g, s);
  DCNN_LAUNCH_CHECK();
}

void dwconv_dgrad(int dt, const void* dy, const void* w, const void* residual, void* dx, DwArgs g, hipStream_t s) {
  dw_require(dt, g, "dwconv_dgrad");
  if (dt == 1) dw_dgrad_t<bf16>(dy, w, residual, dx, dt, g, s);
  else dw_dgrad_t<float>(dy, w, residual, dx, dt, g, s);
  DCNN_LAUNCH_CHECK();
}

int dwconv_wgrad_splits(int dt, DwArgs g) {
  dw_require(dt, g, "dwconv_wgrad_splits");
  return dw_wgrad_splits_k(dw_wgrad_geom(dt, g));
}

void dwconv_wgrad(int dt, const void* dy, const void* x, float* slab, float* bias_slab, DwArgs g, hipStream_t s) {
  dw_require(dt, g, "dwconv_wgrad");
  if (dt == 1) dw_wgrad_t<bf16>(dy, x, slab, bias_slab, dt, g, s);
  else dw_wgrad_t<float>(dy, x, slab, bias_slab, dt, g, s);
  DCNN_LAUNCH_CHECK();
}

}  // namespace dcnn
