// Grouped convolution (1 < groups < C) on NHWC activations: forward, data gradient (gather form)
// and weight gradient (slab per split, reduced by splitk_reduce*). F.conv2d(x, w, groups = G)
// semantics; weights [Co][KH][KW][Cig] (channels_last), Cig = Ci / G, Cog = Co / G.
//
// All three passes are implicit GEMMs on the matrix cores, one launch covering every group:
// mfma_f32_16x16x32_bf16 for bf16, eight mfma_f32_16x16x4f32 per 32-deep step for fp32 (exact
// fp32). No im2col buffer, no LDS in forward / dgrad, no atomics, no scratch.
//
// Forward / dgrad (one kernel template): a wave owns 64 destination pixels x 16 destination
// channels (four 16x16 accumulators sharing one weight fragment); the four waves of a workgroup take
// four adjacent channel tiles of the same pixels, so that together they use whole cache lines of
// each pixel's channels (each alone reads a 16-64 byte slice). The 16-channel tile [n0, n0+16)
// belongs to one group when the destination group size Dg >= 16 and bundles 16 / Dg adjacent
// groups otherwise; its source channels are the contiguous range of those groups. A k-step is
// four "units" — lane block l >> 4 takes unit 4 s + (l >> 4) — and a unit is (tap, 8 consecutive
// source channels): the operand lane map of the 16x16x32 MFMA gives a lane 8 consecutive k of one
// row, i.e. one 16-byte load of 8 channels of one pixel at one tap (two 8-byte loads of 4 channels
// where a chunk is not 16-byte aligned; with a source group size of 4 the two halves of the weight
// chunk belong to different groups and are always loaded separately). The weight fragment
// is block diagonal: a 4-channel half whose source group is not the destination channel's group is
// zero (a select at the load from [Cd][T][Sg]); the waste is at most the bundle factor and the
// small-group shapes are bandwidth-bound. The weight fragment is the A operand and the pixel
// fragment the B operand, so a lane's four accumulator registers are four consecutive channels of
// one pixel: one 8-byte (bf16) / 16-byte (fp32) store, bias or residual added before the single
// rounding. Taps are a run-time loop with per-row bounds predicates: any KH x KW <= 49, any
// stride, any pad < kernel.
// The data gradient is the same GEMM on dy with the transposed operand [Ci][T][Cog]
// (gconv_weight_t, one small launch) and the inverse pixel map: tap (ky, kx) of input row iy reads
// output row (iy + PH - ky) / SH when that division is exact and in range and contributes zero
// otherwise (the zero-tap form for strides > 1). Every input pixel is written exactly once.
//
// Weight gradient: dW[co][t][ci] = sum over pixels dy[p][co] x[p @ t][ci], K = pixels. A workgroup
// is one wave: a 16 (co) x 16 (ci) tile of one bundle, up to 9 taps (grid.y walks tap groups, so
// the accumulators stay in registers), one pixel range (grid.z = split). The MFMA operands need 8
// consecutive k = 8 pixels of one channel per lane, the transpose of NHWC, so each 32-pixel step
// stages dy and the tap-shifted x tiles through LDS ([channel][pixel], rows padded by 16 bytes;
// fragments are single 16-byte reads). A step's global loads (dy and all taps of x) are issued
// before its first barrier, the x tiles then alternate between two LDS buffers, one barrier per
// tap. Only the diagonal blocks of a bundle are written to the
// slab, as 16-byte rows in the weight layout; the bias partial is one more MFMA against a
// fragment of ones. The split -> pixel range map is a pure function of the shape.
#include "api.h"
#include "common.h"

namespace dcnn {
namespace {

constexpr int kGcMaxTaps = 49;
constexpr int kGcTapGroup = 9;     // taps per weight-gradient workgroup
constexpr int kGcMT = 4;           // 16-pixel tiles per wave (forward / dgrad)
constexpr int kGcThreads = 256;
constexpr int kGcWgradWaves = 4096;  // one-wave workgroups the split decision aims for (4 per SIMD)
constexpr int kGcMinSteps = 4;       // least 32-pixel steps per split
constexpr int kGcMaxSplits = 512;
constexpr long kGcSlabBytes = 8l << 20;  // the splits' slabs (written, then read by the reduce) stay below this

// 4-channel half of a fragment as raw bits: 8 bytes of bf16 / 16 bytes of fp32
template <typename T> struct GcT;
template <> struct GcT<bf16> {
  typedef uint2 H;
  typedef unsigned short E;
  static __device__ __forceinline__ H zero() { return make_uint2(0u, 0u); }
  static __device__ __forceinline__ H one() { return make_uint2(0x3F803F80u, 0x3F803F80u); }
  static __device__ __forceinline__ E elem(const H& h, int j) {
    const unsigned u = j < 2 ? h.x : h.y;
    return (E)((j & 1) ? (u >> 16) : (u & 0xffffu));
  }
};
template <> struct GcT<float> {
  typedef f32x4 H;
  typedef float E;
  static __device__ __forceinline__ H zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ H one() { return f32x4{1.f, 1.f, 1.f, 1.f}; }
  static __device__ __forceinline__ E elem(const H& h, int j) { return h[j]; }
};
template <typename T> struct GcFrag {
  typename GcT<T>::H h[2];
};

__device__ __forceinline__ f32x4 gc_mma(const GcFrag<bf16>& a, const GcFrag<bf16>& b, f32x4 c) {
  const uint4 ua = make_uint4(a.h[0].x, a.h[0].y, a.h[1].x, a.h[1].y);
  const uint4 ub = make_uint4(b.h[0].x, b.h[0].y, b.h[1].x, b.h[1].y);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ua), __builtin_bit_cast(bf16x8, ub), c, 0,
                                                 0, 0);
}
__device__ __forceinline__ f32x4 gc_mma(const GcFrag<float>& a, const GcFrag<float>& b, f32x4 c) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.h[h][j], b.h[h][j], c, 0, 0, 0);
  return c;
}

// 8 consecutive channels at p: one 16-byte load when the source is 8-channel aligned (full8, both
// halves share v0), else two predicated 4-channel loads
template <typename T>
__device__ __forceinline__ GcFrag<T> gc_load(const T* p, bool full8, bool v0, bool v1) {
  typedef typename GcT<T>::H H;
  GcFrag<T> f;
  f.h[0] = GcT<T>::zero();
  f.h[1] = GcT<T>::zero();
  if constexpr (std::is_same<T, bf16>::value) {
    if (full8) {
      if (v0) {
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        f.h[0] = make_uint2(u.x, u.y);
        f.h[1] = make_uint2(u.z, u.w);
      }
      return f;
    }
  }
  if (v0) f.h[0] = *reinterpret_cast<const H*>(p);
  if (v1) f.h[1] = *reinterpret_cast<const H*>(p + 4);
  return f;
}

__device__ __forceinline__ void gc_store4(bf16* p, const f32x4& v) {
  bf16x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (bf16)v[j];
  *reinterpret_cast<bf16x4*>(p) = o;
}
__device__ __forceinline__ void gc_store4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ f32x4 gc_load4f(const bf16* p) {
  const bf16x4 o = *reinterpret_cast<const bf16x4*>(p);
  return f32x4{(float)o[0], (float)o[1], (float)o[2], (float)o[3]};
}
__device__ __forceinline__ f32x4 gc_load4f(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// forward / dgrad launch geometry ("source" is the tensor gathered from, "dest" the one written)
struct GcK {
  int P, DH, DW;        // destination pixels N * DH * DW
  int SHt, SWt;         // source map
  int Cs, Cd, Sg, Dg;   // channels and group sizes
  int KH, KW, SH, SW, PH, PW;
  int T, CPT, U;        // taps, 8-channel chunks per tap, units = T * CPT
  int full8, afull8;    // 16-byte loads of 8 channels: weights (Sg % 8 == 0) / activations (aligned chunks)
  FastDiv fdhw, fdw, fkw, fcpt, fdg, fsg;
};

// exact sy / S for sy >= 0 where S divides sy (ok = false otherwise)
__device__ __forceinline__ int gc_unstride(int sy, int S, bool& ok) {
  if (S == 1) return sy;
  if (S == 2) {
    ok = ok && !(sy & 1);
    return sy >> 1;
  }
  const int q = sy / S;
  ok = ok && q * S == sy;
  return q;
}

template <typename T, bool DGRAD>
__global__ __launch_bounds__(kGcThreads) void gconv_kernel(const T* __restrict__ src, const T* __restrict__ wk,
                                                           const float* __restrict__ bias,
                                                           const T* __restrict__ residual, T* __restrict__ dst,
                                                           const GcK k) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kb = lane >> 4;
  // the workgroup's waves take adjacent channel tiles of the same 64 pixels: together they use
  // the whole cache lines of a pixel's channels that each of them reads a slice of
  const int n0 = (blockIdx.y * (kGcThreads / 64) + wave) * 16;
  if (n0 >= k.Cd) return;
  const int d = n0 + r;  // this lane's row of the weight fragment
  const bool dv = d < k.Cd;
  const int gd = (int)fdiv((unsigned)(dv ? d : k.Cd - 1), k.fdg);
  const int c_lo = (int)fdiv((unsigned)n0, k.fdg) * k.Sg;
  const int p0 = blockIdx.x * (16 * kGcMT);
  const bool full8 = k.full8 != 0, afull8 = k.afull8 != 0;

  int pb[kGcMT], by[kGcMT], bx[kGcMT];
  bool pv[kGcMT];
#pragma unroll
  for (int m = 0; m < kGcMT; ++m) {
    const int p = p0 + m * 16 + r;
    pv[m] = p < k.P;
    const unsigned pp = pv[m] ? (unsigned)p : 0u;
    const unsigned n = fdiv(pp, k.fdhw);
    const unsigned rem = pp - n * (unsigned)(k.DH * k.DW);
    const unsigned y = fdiv(rem, k.fdw);
    const unsigned x = rem - y * (unsigned)k.DW;
    pb[m] = (int)n * k.SHt * k.SWt;
    by[m] = DGRAD ? (int)y + k.PH : (int)y * k.SH - k.PH;
    bx[m] = DGRAD ? (int)x + k.PW : (int)x * k.SW - k.PW;
  }
  f32x4 acc[kGcMT];
#pragma unroll
  for (int m = 0; m < kGcMT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nsteps = (k.U + 3) >> 2;
  for (int s = 0; s < nsteps; ++s) {
    const int u = 4 * s + kb;
    const bool uv = u < k.U;
    const int t = (int)fdiv((unsigned)(uv ? u : 0), k.fcpt);
    const int ch = (uv ? u : 0) - t * k.CPT;
    const int ky = (int)fdiv((unsigned)t, k.fkw), kx = t - ky * k.KW;
    const int c0 = c_lo + ch * 8;
    // block-diagonal weight fragment: row d, tap t, source channels c0 .. c0 + 7
    const bool cv0 = c0 + 3 < k.Cs, cv1 = c0 + 7 < k.Cs;
    const bool wv0 = uv && dv && cv0 && (int)fdiv((unsigned)(cv0 ? c0 : 0), k.fsg) == gd;
    const bool wv1 = uv && dv && cv1 && (int)fdiv((unsigned)(cv1 ? c0 + 4 : 0), k.fsg) == gd;
    const int woff = ((dv ? d : 0) * k.T + t) * k.Sg + (c0 - gd * k.Sg);
    const GcFrag<T> wf = gc_load<T>(wk + woff, full8, wv0, wv1);
#pragma unroll
    for (int m = 0; m < kGcMT; ++m) {
      int sy = DGRAD ? by[m] - ky : by[m] + ky;
      int sx = DGRAD ? bx[m] - kx : bx[m] + kx;
      bool ok = pv[m] && uv && sy >= 0 && sx >= 0;
      if (DGRAD) {
        sy = gc_unstride(sy, k.SH, ok);
        sx = gc_unstride(sx, k.SW, ok);
      }
      ok = ok && sy < k.SHt && sx < k.SWt;
      const int off = ok ? (pb[m] + sy * k.SWt + sx) * k.Cs + c0 : 0;
      const GcFrag<T> af = gc_load<T>(src + off, afull8, ok && (afull8 ? cv1 : cv0), ok && cv1);
      acc[m] = gc_mma(wf, af, acc[m]);
    }
  }

  // D[row = channel n0 + 4 kb + j][col = pixel r]
  const int dch = n0 + 4 * kb;
  if (dch >= k.Cd) return;
  f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
  if (bias != nullptr) bv = *reinterpret_cast<const f32x4*>(bias + dch);
#pragma unroll
  for (int m = 0; m < kGcMT; ++m) {
    if (!pv[m]) continue;
    const int o = (p0 + m * 16 + r) * k.Cd + dch;
    f32x4 v = acc[m] + bv;
    if (residual != nullptr) v += gc_load4f(residual + o);
    gc_store4(dst + o, v);
  }
}

// [Co][T][Cig] -> [Ci][T][Cog] (the data gradient's operand)
template <typename T>
__global__ void gconv_weight_t_kernel(const T* __restrict__ w, T* __restrict__ wt, int Ci, int T_, int Cig, int Cog,
                                      int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int col = i % Cog;
  const int t = (i / Cog) % T_;
  const int ci = i / (Cog * T_);
  const int g = ci / Cig;
  wt[i] = w[((g * Cog + col) * T_ + t) * Cig + (ci - g * Cig)];
}

struct GwK {
  int P, OH, OW, H, W, Ci, Co, Cig, Cog, KH, KW, SH, SW, PH, PW;
  int T, NCT, ksteps, per_split, n;  // n = Co * T * Cig (slab row)
  FastDiv fohw, fow, fkw, fcig, fcog, fnct;
};

template <typename T>
__global__ __launch_bounds__(64) void gconv_wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                         float* __restrict__ slab, float* __restrict__ bslab,
                                                         const GwK k) {
  typedef typename GcT<T>::H H;
  typedef typename GcT<T>::E E;
  constexpr int LS = 32 + 16 / (int)sizeof(T);  // [channel][32 pixels + 16 bytes]
  __shared__ __attribute__((aligned(16))) E lds[3][16][LS];  // 0: dy, 1 / 2: x at alternating taps

  const int lane = threadIdx.x;
  const int r = lane & 15, kb = lane >> 4;
  const int q = lane & 3, pl = lane >> 2;  // staging: channel quad, pixel (and pixel + 16)
  const int cot = (int)fdiv(blockIdx.x, k.fnct), cit = (int)blockIdx.x - cot * k.NCT;
  const int co0 = cot * 16;
  const int g_lo = (int)fdiv((unsigned)co0, k.fcog);
  const int g_hi = (int)fdiv((unsigned)min(co0 + 15, k.Co - 1), k.fcog);
  const int ci0 = g_lo * k.Cig + cit * 16;
  if (ci0 >= (g_hi + 1) * k.Cig) return;  // (uniform) a partly empty last bundle
  const int t0 = blockIdx.y * kGcTapGroup;
  const int split = blockIdx.z;
  const bool do_bias = bslab != nullptr && blockIdx.y == 0 && cit == 0;
  const bool yv = co0 + 4 * q < k.Co, xv_ok = ci0 + 4 * q < k.Ci;

  f32x4 acc[kGcTapGroup];
#pragma unroll
  for (int i = 0; i < kGcTapGroup; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 accb = f32x4{0.f, 0.f, 0.f, 0.f};
  GcFrag<T> ones;
  ones.h[0] = GcT<T>::one();
  ones.h[1] = GcT<T>::one();

  const int ks1 = min((split + 1) * k.per_split, k.ksteps);
  for (int ks = split * k.per_split; ks < ks1; ++ks) {
    int xb[2], iy0[2], ix0[2];
    H dv[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int p = ks * 32 + pl + 16 * e;
      const bool pv = p < k.P;
      const unsigned pp = pv ? (unsigned)p : 0u;
      const unsigned n = fdiv(pp, k.fohw);
      const unsigned rem = pp - n * (unsigned)(k.OH * k.OW);
      const unsigned oy = fdiv(rem, k.fow);
      const unsigned ox = rem - oy * (unsigned)k.OW;
      xb[e] = (int)n * k.H * k.W;
      iy0[e] = pv ? (int)oy * k.SH - k.PH : -(1 << 20);
      ix0[e] = (int)ox * k.SW - k.PW;
      dv[e] = GcT<T>::zero();
      if (pv && yv) dv[e] = *reinterpret_cast<const H*>(dy + (int)pp * k.Co + co0 + 4 * q);
    }
    // every tap's x vectors before the first barrier: one round of global latency per step
    H xv[kGcTapGroup][2];
#pragma unroll
    for (int i = 0; i < kGcTapGroup; ++i) {
      const int t = t0 + i < k.T ? t0 + i : 0;
      const int ky = (int)fdiv((unsigned)t, k.fkw), kx = t - ky * k.KW;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int iy = iy0[e] + ky, ix = ix0[e] + kx;
        xv[i][e] = GcT<T>::zero();
        if (t0 + i < k.T && xv_ok && iy >= 0 && iy < k.H && ix >= 0 && ix < k.W)
          xv[i][e] = *reinterpret_cast<const H*>(x + (xb[e] + iy * k.W + ix) * k.Ci + ci0 + 4 * q);
      }
    }
    __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int j = 0; j < 4; ++j) lds[0][4 * q + j][pl + 16 * e] = GcT<T>::elem(dv[e], j);
    GcFrag<T> yf;
#pragma unroll
    for (int i = 0; i < kGcTapGroup; ++i) {
      const int t = t0 + i;
      if (t < k.T) {  // (uniform)
        E(*buf)[LS] = lds[1 + (i & 1)];
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
          for (int j = 0; j < 4; ++j) buf[4 * q + j][pl + 16 * e] = GcT<T>::elem(xv[i][e], j);
        __syncthreads();
        if (i == 0) {
          yf.h[0] = *reinterpret_cast<const H*>(&lds[0][r][8 * kb]);
          yf.h[1] = *reinterpret_cast<const H*>(&lds[0][r][8 * kb + 4]);
        }
        GcFrag<T> xf;
        xf.h[0] = *reinterpret_cast<const H*>(&buf[r][8 * kb]);
        xf.h[1] = *reinterpret_cast<const H*>(&buf[r][8 * kb + 4]);
        acc[i] = gc_mma(xf, yf, acc[i]);  // D[row = ci][col = co]
        if (i == 0 && do_bias) accb = gc_mma(ones, yf, accb);
      }
    }
  }

  const int co = co0 + r, ci = ci0 + 4 * kb;
  if (co >= k.Co) return;
  const int gco = (int)fdiv((unsigned)co, k.fcog);
  if (do_bias && kb == 0) bslab[split * k.Co + co] = accb[0];
  if (ci >= k.Ci || (int)fdiv((unsigned)ci, k.fcig) != gco) return;  // off-diagonal block of the bundle
  float* out = slab + (long)split * k.n + (co * k.T) * k.Cig + (ci - gco * k.Cig);
#pragma unroll
  for (int i = 0; i < kGcTapGroup; ++i)
    if (t0 + i < k.T) *reinterpret_cast<f32x4*>(out + (t0 + i) * k.Cig) = acc[i];
}

bool gc_size_ok(int c) { return c == 4 || c == 8 || c == 16 || (c >= 32 && c % 32 == 0); }

void gc_require(int dt, const GcArgs& g, const char* what) {
  if (!gconv_supported(dt, g)) throw std::invalid_argument(std::string(what) + ": unsupported grouped conv shape");
}

GcK gc_geom(const GcArgs& g, bool dgrad) {
  GcK k{};
  k.DH = dgrad ? g.H : g.OH;
  k.DW = dgrad ? g.W : g.OW;
  k.SHt = dgrad ? g.OH : g.H;
  k.SWt = dgrad ? g.OW : g.W;
  k.P = g.N * k.DH * k.DW;
  k.Cs = dgrad ? g.Co : g.Ci;
  k.Cd = dgrad ? g.Ci : g.Co;
  k.Sg = k.Cs / g.G;
  k.Dg = k.Cd / g.G;
  k.KH = g.KH; k.KW = g.KW; k.SH = g.SH; k.SW = g.SW; k.PH = g.PH; k.PW = g.PW;
  k.T = g.KH * g.KW;
  const int bundle = k.Dg >= 16 ? 1 : 16 / k.Dg;  // groups per 16-channel destination tile
  k.CPT = (bundle * k.Sg + 7) / 8;
  k.U = k.T * k.CPT;
  k.full8 = k.Sg % 8 == 0;
  k.afull8 = k.Cs % 8 == 0 && (bundle * k.Sg) % 8 == 0;  // every tile's first source channel is 8-aligned
  k.fdhw = make_fastdiv((unsigned)(k.DH * k.DW));
  k.fdw = make_fastdiv((unsigned)k.DW);
  k.fkw = make_fastdiv((unsigned)g.KW);
  k.fcpt = make_fastdiv((unsigned)k.CPT);
  k.fdg = make_fastdiv((unsigned)k.Dg);
  k.fsg = make_fastdiv((unsigned)k.Sg);
  return k;
}

template <typename T>
void gc_launch(bool dgrad, const void* src, const void* wk, const float* bias, const void* residual, void* dst,
               const GcK& k, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(k.P, 16 * kGcMT), (unsigned)ceil_div(k.Cd, 16 * (kGcThreads / 64)));
  if (dgrad)
    hipLaunchKernelGGL((gconv_kernel<T, true>), grid, dim3(kGcThreads), 0, s, (const T*)src, (const T*)wk, bias,
                       (const T*)residual, (T*)dst, k);
  else
    hipLaunchKernelGGL((gconv_kernel<T, false>), grid, dim3(kGcThreads), 0, s, (const T*)src, (const T*)wk, bias,
                       (const T*)residual, (T*)dst, k);
  DCNN_LAUNCH_CHECK();
}

GwK gw_geom(const GcArgs& g) {
  GwK k{};
  k.P = g.N * g.OH * g.OW;
  k.OH = g.OH; k.OW = g.OW; k.H = g.H; k.W = g.W; k.Ci = g.Ci; k.Co = g.Co;
  k.Cig = g.Ci / g.G;
  k.Cog = g.Co / g.G;
  k.KH = g.KH; k.KW = g.KW; k.SH = g.SH; k.SW = g.SW; k.PH = g.PH; k.PW = g.PW;
  k.T = g.KH * g.KW;
  const int bundle = k.Cog >= 16 ? 1 : 16 / k.Cog;
  k.NCT = (bundle * k.Cig + 15) / 16;
  k.ksteps = ceil_div(k.P, 32);
  const int tiles = ceil_div(g.Co, 16) * k.NCT * ceil_div(k.T, kGcTapGroup);
  int splits = kGcWgradWaves / tiles;
  if (splits > k.ksteps / kGcMinSteps) splits = k.ksteps / kGcMinSteps;
  k.n = g.Co * k.T * k.Cig;
  if (splits > kGcMaxSplits) splits = kGcMaxSplits;
  if ((long)splits * k.n * 4 > kGcSlabBytes) splits = (int)(kGcSlabBytes / ((long)k.n * 4));
  if (splits < 1) splits = 1;
  k.per_split = ceil_div(k.ksteps, splits);
  k.fohw = make_fastdiv((unsigned)(g.OH * g.OW));
  k.fow = make_fastdiv((unsigned)g.OW);
  k.fkw = make_fastdiv((unsigned)g.KW);
  k.fcig = make_fastdiv((unsigned)k.Cig);
  k.fcog = make_fastdiv((unsigned)k.Cog);
  k.fnct = make_fastdiv((unsigned)k.NCT);
  return k;
}

}  // namespace

bool gconv_supported(int dt, GcArgs g) {
  if (dt != 0 && dt != 1) return false;
  if (g.N < 1 || g.H < 1 || g.W < 1 || g.Ci < 1 || g.Co < 1 || g.G < 2 || g.Ci % g.G || g.Co % g.G) return false;
  if (!gc_size_ok(g.Ci / g.G) || !gc_size_ok(g.Co / g.G)) return false;
  if (g.KH < 1 || g.KW < 1 || g.KH * g.KW > kGcMaxTaps || g.SH < 1 || g.SW < 1) return false;
  if (g.PH < 0 || g.PW < 0 || g.PH >= g.KH || g.PW >= g.KW) return false;
  if (g.H + 2 * g.PH < g.KH || g.W + 2 * g.PW < g.KW) return false;
  if (g.OH != (g.H + 2 * g.PH - g.KH) / g.SH + 1 || g.OW != (g.W + 2 * g.PW - g.KW) / g.SW + 1) return false;
  const long lim = (1l << 31) - (1l << 16);  // (tile overhang of the pixel index stays below 2^31)
  if ((long)g.N * g.H * g.W * g.Ci >= lim || (long)g.N * g.OH * g.OW * g.Co >= lim) return false;
  if ((long)g.Co * g.KH * g.KW * (g.Ci / g.G) >= lim) return false;
  return true;
}

void gconv_fwd(int dt, const void* x, const void* w, const float* bias, void* y, GcArgs g, hipStream_t s) {
  gc_require(dt, g, "gconv_fwd");
  const GcK k = gc_geom(g, false);
  if (dt == 1) gc_launch<bf16>(false, x, w, bias, nullptr, y, k, s);
  else gc_launch<float>(false, x, w, bias, nullptr, y, k, s);
}

void gconv_weight_t(int dt, const void* w, void* wt, GcArgs g, hipStream_t s) {
  gc_require(dt, g, "gconv_weight_t");
  const int T_ = g.KH * g.KW, Cig = g.Ci / g.G, Cog = g.Co / g.G, total = g.Ci * T_ * Cog;
  const dim3 grid((unsigned)ceil_div(total, 256));
  if (dt == 1)
    hipLaunchKernelGGL(gconv_weight_t_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)w, (bf16*)wt, g.Ci, T_, Cig,
                       Cog, total);
  else
    hipLaunchKernelGGL(gconv_weight_t_kernel<float>, grid, dim3(256), 0, s, (const float*)w, (float*)wt, g.Ci, T_, Cig,
                       Cog, total);
  DCNN_LAUNCH_CHECK();
}

void gconv_dgrad(int dt, const void* dy, const void* wt, const void* residual, void* dx, GcArgs g, hipStream_t s) {
  gc_require(dt, g, "gconv_dgrad");
  const GcK k = gc_geom(g, true);
  if (dt == 1) gc_launch<bf16>(true, dy, wt, nullptr, residual, dx, k, s);
  else gc_launch<float>(true, dy, wt, nullptr, residual, dx, k, s);
}

int gconv_wgrad_splits(int dt, GcArgs g) {
  gc_require(dt, g, "gconv_wgrad_splits");
  const GwK k = gw_geom(g);
  return ceil_div(k.ksteps, k.per_split);
}

void gconv_wgrad(int dt, const void* dy, const void* x, float* slab, float* bias_slab, GcArgs g, hipStream_t s) {
  gc_require(dt, g, "gconv_wgrad");
  const GwK k = gw_geom(g);
  const int splits = ceil_div(k.ksteps, k.per_split);
  const dim3 grid((unsigned)(ceil_div(g.Co, 16) * k.NCT), (unsigned)ceil_div(k.T, kGcTapGroup), (unsigned)splits);
  if (dt == 1)
    hipLaunchKernelGGL(gconv_wgrad_kernel<bf16>, grid, dim3(64), 0, s, (const bf16*)dy, (const bf16*)x, slab,
                       bias_slab, k);
  else
    hipLaunchKernelGGL(gconv_wgrad_kernel<float>, grid, dim3(64), 0, s, (const float*)dy, (const float*)x, slab,
                       bias_slab, k);
  DCNN_LAUNCH_CHECK();
}

}  // namespace dcnn
