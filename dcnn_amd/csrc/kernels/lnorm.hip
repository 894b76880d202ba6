// Channel LayerNorm and LayerScale on NHWC activations (bf16 or fp32 I/O, fp32 arithmetic).
//
// The activation is R = N*H*W rows of C contiguous channels. No reference counterpart (the
// reference has neither layer); semantics are F.layer_norm over the last dimension and a
// per-channel multiply.
//
// Lane mapping. A row is owned by a group of G lanes, G a power of two, so one wave works on
// 64 / G rows at once and a 256-thread workgroup on 256 / G. A lane moves VPL 16-byte vectors
// (8 bf16 or 4 fp32) per row: vector j = lane_in_group + k * G, k < VPL. With nvec = C / 8 (bf16)
// or C / 4 (fp32) vectors per row, VPL = 1 and G = the next power of two >= nvec while nvec <= 64,
// else G = 64 and VPL = 2, 4 or (fp32 only, C > 1024) 8. Lanes whose
// vector index is >= nvec are inactive: they load nothing, add zeros to the row sums and store
// nothing. Lane utilisation is nvec / (G * VPL): 12 / 16 = 75 % at C = 96 in bf16 (24 / 32 and
// 48 / 64 at C = 192 and 384 likewise), 100 % at every power-of-two vector count.
//
// Forward: the lane's share of the row is loaded once and stays in registers through the mean,
// the centred sum of squares (x - mean)^2 (never E[x^2] - mean^2) and the apply. Backward: dy and
// x are loaded once each. Row sums are xor-butterflies over the G lanes of the group; every lane
// of the group ends with the same bits.
//
// dgamma / dbeta (and LayerScale's dgamma): each lane keeps fp32 partial sums for its own
// channels over all the rows it visits; at the end the 64 / G groups of a wave are summed by a
// fixed butterfly, the four waves through LDS in wave order, and the workgroup writes one slab
// row ([2][C], LayerScale [C]). ln_slab_reduce_kernel sums the slab rows in a fixed order and
// adds to the gradients (the project's accumulate convention). No float atomics: results are
// bit-identical from run to run. The grid is capped (2048 workgroups forward, 1024 backward) with
// a loop over row groups; the slab comes from the caller; nothing here allocates or synchronises.
//
// lscale_drop_fwd / lscale_drop_bwd are the LayerScale pair with a stochastic-depth mask (one
// float per sample, droppath.hip) folded in, for a residual block closing in LayerScale, DropPath
// (RF_DROP_TAIL): kernels of their own beside lscale_fwd / lscale_bwd, same lane mapping, same slab
// and reduce. A dropped sample's rows copy the residual (forward) or are zeros (backward) and its
// x / dy rows are never loaded.
#include <algorithm>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "common.h"
#include "api.h"

namespace dcnn {
namespace lnorm {  // (a named namespace: kernel traces show dcnn::lnorm::ln_fwd_kernel<...>)

constexpr int kLnFwdGridCap = 2048;  // 8 workgroups per CU
constexpr int kLnBwdGridCap = 1024;  // 4 per CU: the slab stays <= 1024 rows

template <typename T>
struct LnVec;
template <>
struct LnVec<bf16> {
  static constexpr int V = 8;
  __device__ static __forceinline__ void load(const bf16* p, float* f) {
    unpack8(*reinterpret_cast<const uint4*>(p), f);
  }
  __device__ static __forceinline__ void store(bf16* p, const float* f) {
    *reinterpret_cast<uint4*>(p) = pack8(f);
  }
};
template <>
struct LnVec<float> {
  static constexpr int V = 4;
  __device__ static __forceinline__ void load(const float* p, float* f) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  }
  __device__ static __forceinline__ void store(float* p, const float* f) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  }
};

// sum over the G lanes that own a row (all lanes of the wave take part)
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// per-channel parameter vector of this lane (fill where absent or the lane is inactive)
template <int VPL, int V, int G>
__device__ __forceinline__ void load_param(const float* __restrict__ p, int g, int C, float fill, float (&out)[VPL][V]) {
#pragma unroll
  for (int k = 0; k < VPL; ++k) {
    const int c = (g + k * G) * V;
#pragma unroll
    for (int v = 0; v < V; v += 4) {
      float4 a = make_float4(fill, fill, fill, fill);
      if (p && c < C) a = *reinterpret_cast<const float4*>(p + c + v);
      out[k][v] = a.x; out[k][v + 1] = a.y; out[k][v + 2] = a.z; out[k][v + 3] = a.w;
    }
  }
}

// Workgroup sum of the per-lane channel partials acc (channel (g + k G) V + v of lane group g):
// the 64 / G groups of each wave by a fixed butterfly, then the 4 waves through sh [4][G VPL V]
// in wave order; out[c], c < C.
template <int VPL, int V, int G>
__device__ __forceinline__ void wg_channel_sum(float (&acc)[VPL][V], float* sh, float* __restrict__ out, int C) {
  constexpr int CG = G * VPL * V;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < VPL; ++k)
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int o = G; o < 64; o <<= 1) acc[k][v] += __shfl_xor(acc[k][v], o, 64);
  __syncthreads();  // sh is free again
  if (lane < G) {
#pragma unroll
    for (int k = 0; k < VPL; ++k)
#pragma unroll
      for (int v = 0; v < V; v += 4)
        *reinterpret_cast<float4*>(sh + wave * CG + (lane + k * G) * V + v) =
            make_float4(acc[k][v], acc[k][v + 1], acc[k][v + 2], acc[k][v + 3]);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) out[c] = ((sh[c] + sh[CG + c]) + sh[2 * CG + c]) + sh[3 * CG + c];
}

template <typename T, int VPL, int G>
__global__ void __launch_bounds__(256) ln_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int R, int C,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float eps, float* __restrict__ save_mean,
                                                     float* __restrict__ save_rstd) {
  constexpr int V = LnVec<T>::V, RPB = 256 / G;
  const int g = threadIdx.x % G, sub = threadIdx.x / G;
  const float inv_c = 1.f / (float)C;
  float gm[VPL][V], bt[VPL][V];
  load_param<VPL, V, G>(gamma, g, C, 1.f, gm);
  load_param<VPL, V, G>(beta, g, C, 0.f, bt);
  for (int row0 = blockIdx.x * RPB; row0 < R; row0 += gridDim.x * RPB) {
    const int row = row0 + sub;
    const bool ok = row < R;
    const long base = (long)row * C;
    float f[VPL][V];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int c = (g + k * G) * V;
      if (ok && c < C) {
        LnVec<T>::load(x + base + c, f[k]);
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) f[k][v] = 0.f;
      }
#pragma unroll
      for (int v = 0; v < V; ++v) s += f[k][v];
    }
    const float mean = group_sum<G>(s) * inv_c;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const bool act = (g + k * G) * V < C;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        f[k][v] -= mean;
        q += act ? f[k][v] * f[k][v] : 0.f;
      }
    }
    const float rstd = rsqrtf(group_sum<G>(q) * inv_c + eps);
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int c = (g + k * G) * V;
      if (ok && c < C) {
        float o[V];
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] = f[k][v] * rstd * gm[k][v] + bt[k][v];
        LnVec<T>::store(y + base + c, o);
      }
    }
    if (ok && g == 0) {
      if (save_mean) save_mean[row] = mean;
      if (save_rstd) save_rstd[row] = rstd;
    }
  }
}

// slab row [2][C] of this workgroup = (sum dy xhat, sum dy) when slab is set
template <typename T, int VPL, int G>
__global__ void __launch_bounds__(256) ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                     T* __restrict__ dx, int R, int C, const float* __restrict__ gamma,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     float* __restrict__ slab) {
  constexpr int V = LnVec<T>::V, RPB = 256 / G;
  __shared__ __attribute__((aligned(16))) float sh[4 * G * VPL * V];
  const int g = threadIdx.x % G, sub = threadIdx.x / G;
  const float inv_c = 1.f / (float)C;
  float gm[VPL][V], ag[VPL][V], ab[VPL][V];
  load_param<VPL, V, G>(gamma, g, C, 1.f, gm);
#pragma unroll
  for (int k = 0; k < VPL; ++k)
#pragma unroll
    for (int v = 0; v < V; ++v) ag[k][v] = ab[k][v] = 0.f;
  for (int row0 = blockIdx.x * RPB; row0 < R; row0 += gridDim.x * RPB) {
    const int row = row0 + sub;
    const bool ok = row < R;
    const long base = (long)row * C;
    const float mu = ok ? mean[row] : 0.f, rs = ok ? rstd[row] : 0.f;
    float d[VPL][V], xh[VPL][V];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int c = (g + k * G) * V;
      if (ok && c < C) {
        LnVec<T>::load(dy + base + c, d[k]);
        LnVec<T>::load(x + base + c, xh[k]);
#pragma unroll
        for (int v = 0; v < V; ++v) xh[k][v] = (xh[k][v] - mu) * rs;
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) d[k][v] = xh[k][v] = 0.f;
      }
#pragma unroll
      for (int v = 0; v < V; ++v) {
        ag[k][v] += d[k][v] * xh[k][v];
        ab[k][v] += d[k][v];
        d[k][v] *= gm[k][v];
        s1 += d[k][v];
        s2 += d[k][v] * xh[k][v];
      }
    }
    const float m1 = group_sum<G>(s1) * inv_c, m2 = group_sum<G>(s2) * inv_c;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int c = (g + k * G) * V;
      if (ok && c < C) {
        float o[V];
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] = rs * (d[k][v] - m1 - xh[k][v] * m2);
        LnVec<T>::store(dx + base + c, o);
      }
    }
  }
  if (slab) {
    float* out = slab + (long)blockIdx.x * 2 * C;
    wg_channel_sum<VPL, V, G>(ag, sh, out, C);
    wg_channel_sum<VPL, V, G>(ab, sh, out + C, C);
  }
}

// y = gamma[c] x (+ residual), elementwise over 16-byte vectors
template <typename T, bool RES>
__global__ void __launch_bounds__(256) lscale_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                         const T* __restrict__ res, T* __restrict__ y, unsigned nv,
                                                         unsigned nvec) {
  constexpr int V = LnVec<T>::V;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < nv; i += gridDim.x * 256u) {
    const unsigned c = (i % nvec) * V;
    float f[V], r[V];
    LnVec<T>::load(x + (size_t)i * V, f);
    if (RES) LnVec<T>::load(res + (size_t)i * V, r);
#pragma unroll
    for (int v = 0; v < V; v += 4) {
      const float4 a = *reinterpret_cast<const float4*>(gamma + c + v);
      f[v] *= a.x; f[v + 1] *= a.y; f[v + 2] *= a.z; f[v + 3] *= a.w;
    }
    if (RES) {
#pragma unroll
      for (int v = 0; v < V; ++v) f[v] += r[v];
    }
    LnVec<T>::store(y + (size_t)i * V, f);
  }
}

// dx = gamma[c] dy; slab row [C] of this workgroup = sum dy x
template <typename T, int VPL, int G>
__global__ void __launch_bounds__(256) lscale_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                         const float* __restrict__ gamma, T* __restrict__ dx, int R,
                                                         int C, float* __restrict__ slab) {
  constexpr int V = LnVec<T>::V, RPB = 256 / G;
  __shared__ __attribute__((aligned(16))) float sh[4 * G * VPL * V];
  const int g = threadIdx.x % G, sub = threadIdx.x / G;
  float gm[VPL][V], ag[VPL][V];
  load_param<VPL, V, G>(gamma, g, C, 1.f, gm);
#pragma unroll
  for (int k = 0; k < VPL; ++k)
#pragma unroll
    for (int v = 0; v < V; ++v) ag[k][v] = 0.f;
  for (int row0 = blockIdx.x * RPB; row0 < R; row0 += gridDim.x * RPB) {
    const int row = row0 + sub;
    const long base = (long)row * C;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int c = (g + k * G) * V;
      if (row < R && c < C) {
        float d[V], xv[V];
        LnVec<T>::load(dy + base + c, d);
        LnVec<T>::load(x + base + c, xv);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          ag[k][v] += d[v] * xv[v];
          d[v] *= gm[k][v];
        }
        LnVec<T>::store(dx + base + c, d);
      }
    }
  }
  wg_channel_sum<VPL, V, G>(ag, sh, slab + (long)blockIdx.x * C, C);
}

// The scale tail with stochastic depth: y = res + (mask[n] gamma[c]) x, n the sample of the row
// (vps vectors per sample). A dropped sample (mask 0) copies its residual rows and never reads x.
// A kernel of its own: lscale_fwd_kernel keeps its code. With mask = 1 the products are the same
// operations in the same order, so the bits equal lscale_fwd's.
template <typename T>
__global__ void __launch_bounds__(256) lscale_drop_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                              const float* __restrict__ mask,
                                                              const T* __restrict__ res, T* __restrict__ y, unsigned nv,
                                                              unsigned nvec, FastDiv vps) {
  constexpr int V = LnVec<T>::V;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < nv; i += gridDim.x * 256u) {
    const float m = mask[fdiv(i, vps)];
    float f[V], r[V];
    LnVec<T>::load(res + (size_t)i * V, r);
    if (m != 0.f) {
      const unsigned c = (i % nvec) * V;
      LnVec<T>::load(x + (size_t)i * V, f);
#pragma unroll
      for (int v = 0; v < V; v += 4) {
        const float4 a = *reinterpret_cast<const float4*>(gamma + c + v);
        f[v] *= a.x * m; f[v + 1] *= a.y * m; f[v + 2] *= a.z * m; f[v + 3] *= a.w * m;
      }
#pragma unroll
      for (int v = 0; v < V; ++v) f[v] += r[v];
      LnVec<T>::store(y + (size_t)i * V, f);
    } else {
      LnVec<T>::store(y + (size_t)i * V, r);
    }
  }
}

// dx = (mask[n] gamma[c]) dy; slab row [C] of this workgroup = sum (mask[n] dy) x. A dropped
// sample's rows are written as zeros and neither dy nor x is read.
template <typename T, int VPL, int G>
__global__ void __launch_bounds__(256) lscale_drop_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ mask, T* __restrict__ dx, int R,
                                                              int C, FastDiv rps, float* __restrict__ slab) {
  constexpr int V = LnVec<T>::V, RPB = 256 / G;
  __shared__ __attribute__((aligned(16))) float sh[4 * G * VPL * V];
  const int g = threadIdx.x % G, sub = threadIdx.x / G;
  float gm[VPL][V], ag[VPL][V];
  load_param<VPL, V, G>(gamma, g, C, 1.f, gm);
#pragma unroll
  for (int k = 0; k < VPL; ++k)
#pragma unroll
    for (int v = 0; v < V; ++v) ag[k][v] = 0.f;
  for (int row0 = blockIdx.x * RPB; row0 < R; row0 += gridDim.x * RPB) {
    const int row = row0 + sub;
    const long base = (long)row * C;
    const float m = row < R ? mask[fdiv((unsigned)row, rps)] : 0.f;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int c = (g + k * G) * V;
      if (row < R && c < C) {
        float d[V];
        if (m != 0.f) {
          float xv[V];
          LnVec<T>::load(dy + base + c, d);
          LnVec<T>::load(x + base + c, xv);
#pragma unroll
          for (int v = 0; v < V; ++v) {
            d[v] *= m;
            ag[k][v] += d[v] * xv[v];
            d[v] *= gm[k][v];
          }
        } else {
#pragma unroll
          for (int v = 0; v < V; ++v) d[v] = 0.f;
        }
        LnVec<T>::store(dx + base + c, d);
      }
    }
  }
  wg_channel_sum<VPL, V, G>(ag, sh, slab + (long)blockIdx.x * C, C);
}

// out[col] += sum over slab rows of slab[row][col], col < n = parts * C; part p adds into o0 / o1.
// One workgroup per 16 columns: 16 row slices (slice q owns rows q, q + 16, ...), each summed into 8
// accumulators (row k of every 8 goes to accumulator k: eight independent loads in flight instead
// of one dependent chain per slab row), combined in a fixed tree, then the slices in slice order.
// (64 slices of 4 columns measured no faster.)
__global__ void __launch_bounds__(256) ln_slab_reduce_kernel(const float* __restrict__ slab, int rows, int n, int C,
                                                             float* __restrict__ o0, float* __restrict__ o1) {
  __shared__ float sh[16][17];
  const int cl = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + cl;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (col < n) {
    int r = q;
    for (; r + 7 * 16 < rows; r += 8 * 16) {
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] += slab[(long)(r + 16 * k) * n + col];
    }
#pragma unroll
    for (int k = 0; k < 7; ++k)  // at most 7 rows are left
      if (r + 16 * k < rows) a[k] += slab[(long)(r + 16 * k) * n + col];
  }
  sh[q][cl] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (q == 0 && col < n) {
    float t = sh[0][cl];
#pragma unroll
    for (int j = 1; j < 16; ++j) t += sh[j][cl];
    float* dst = col < C ? o0 : o1;
    if (dst) dst[col < C ? col : col - C] += t;
  }
}

struct LnShape {
  int VPL, G;
};
LnShape ln_shape(int dt, int C) {
  const int nvec = C / (dt == 1 ? 8 : 4);
  LnShape s{1, 1};
  while (nvec > 64 * s.VPL) s.VPL *= 2;
  if (s.VPL > 1) s.G = 64;
  else
    while (s.G < nvec) s.G *= 2;
  return s;
}

void ln_check(const char* what, int dt, long R, int C) {
  if (!ln_supported(dt, R, C))
    throw std::invalid_argument(std::string(what) + ": unsupported shape: R=" + std::to_string(R) + " rows of C=" +
                                std::to_string(C) + " channels, dtype code " + std::to_string(dt) +
                                " (needs C % " + (dt == 1 ? "8" : "4") + " == 0, 8 <= C <= 2048, R * C < 2^31)");
}

template <int N>
using IC = std::integral_constant<int, N>;

// calls f(IC<VPL>, IC<G>) for the run-time lane shape (VPL = 8: fp32 only, C > 1024)
template <typename T, typename F>
void ln_dispatch(LnShape sh, F&& f) {
  if constexpr (std::is_same<T, float>::value)
    if (sh.VPL == 8) return f(IC<8>{}, IC<64>{});
  if (sh.VPL == 4) return f(IC<4>{}, IC<64>{});
  if (sh.VPL == 2) return f(IC<2>{}, IC<64>{});
  switch (sh.G) {
    case 1: return f(IC<1>{}, IC<1>{});
    case 2: return f(IC<1>{}, IC<2>{});
    case 4: return f(IC<1>{}, IC<4>{});
    case 8: return f(IC<1>{}, IC<8>{});
    case 16: return f(IC<1>{}, IC<16>{});
    case 32: return f(IC<1>{}, IC<32>{});
    default: return f(IC<1>{}, IC<64>{});
  }
}

int ln_groups(int dt, long R, int C) {
  const int rpb = 256 / ln_shape(dt, C).G;
  return (int)((R + rpb - 1) / rpb);
}

template <typename T>
void ln_fwd_t(const void* x, void* y, long R, int C, const float* gamma, const float* beta, float eps,
              float* save_mean, float* save_rstd, hipStream_t s) {
  const int dt = std::is_same<T, bf16>::value ? 1 : 0;
  const int grid = std::min(ln_groups(dt, R, C), kLnFwdGridCap);
  ln_dispatch<T>(ln_shape(dt, C), [&](auto vpl, auto g) {
    ln_fwd_kernel<T, decltype(vpl)::value, decltype(g)::value><<<dim3(grid), dim3(256), 0, s>>>(
        (const T*)x, (T*)y, (int)R, C, gamma, beta, eps, save_mean, save_rstd);
  });
  DCNN_LAUNCH_CHECK();
}

void ln_slab_reduce(const float* slab, int rows, int parts, int C, float* o0, float* o1, hipStream_t s) {
  const int n = parts * C;
  ln_slab_reduce_kernel<<<dim3((n + 15) / 16), dim3(256), 0, s>>>(slab, rows, n, C, o0, o1);
  DCNN_LAUNCH_CHECK();
}

template <typename T>
void ln_bwd_t(const void* dy, const void* x, void* dx, long R, int C, const float* gamma, const float* mean,
              const float* rstd, float* dgamma, float* dbeta, float* workspace, hipStream_t s) {
  const int dt = std::is_same<T, bf16>::value ? 1 : 0;
  const int grid = ln_partial_rows(R, C);
  float* slab = (dgamma || dbeta) ? workspace : nullptr;
  ln_dispatch<T>(ln_shape(dt, C), [&](auto vpl, auto g) {
    ln_bwd_kernel<T, decltype(vpl)::value, decltype(g)::value><<<dim3(grid), dim3(256), 0, s>>>(
        (const T*)dy, (const T*)x, (T*)dx, (int)R, C, gamma, mean, rstd, slab);
  });
  DCNN_LAUNCH_CHECK();
  if (slab) ln_slab_reduce(slab, grid, 2, C, dgamma, dbeta, s);
}

template <typename T>
void lscale_fwd_t(const void* x, const float* gamma, const void* residual, void* y, long R, int C, hipStream_t s) {
  constexpr int V = LnVec<T>::V;
  const unsigned nv = (unsigned)(R * C / V);
  const int grid = grid_for(nv, 256, kLnFwdGridCap);
  if (residual)
    lscale_fwd_kernel<T, true><<<dim3(grid), dim3(256), 0, s>>>((const T*)x, gamma, (const T*)residual, (T*)y, nv,
                                                               (unsigned)(C / V));
  else
    lscale_fwd_kernel<T, false><<<dim3(grid), dim3(256), 0, s>>>((const T*)x, gamma, nullptr, (T*)y, nv,
                                                                (unsigned)(C / V));
  DCNN_LAUNCH_CHECK();
}

template <typename T>
void lscale_bwd_t(const void* dy, const void* x, const float* gamma, void* dx, float* dgamma, long R, int C,
                  float* workspace, hipStream_t s) {
  const int dt = std::is_same<T, bf16>::value ? 1 : 0;
  const int grid = ln_partial_rows(R, C);
  ln_dispatch<T>(ln_shape(dt, C), [&](auto vpl, auto g) {
    lscale_bwd_kernel<T, decltype(vpl)::value, decltype(g)::value><<<dim3(grid), dim3(256), 0, s>>>(
        (const T*)dy, (const T*)x, gamma, (T*)dx, (int)R, C, workspace);
  });
  DCNN_LAUNCH_CHECK();
  ln_slab_reduce(workspace, grid, 1, C, dgamma, nullptr, s);
}

template <typename T>
void lscale_drop_fwd_t(const void* x, const float* gamma, const float* mask, const void* residual, void* y, long R,
                       int C, long rps, hipStream_t s) {
  constexpr int V = LnVec<T>::V;
  const unsigned nv = (unsigned)(R * C / V);
  const int grid = grid_for(nv, 256, kLnFwdGridCap);
  lscale_drop_fwd_kernel<T><<<dim3(grid), dim3(256), 0, s>>>((const T*)x, gamma, mask, (const T*)residual, (T*)y, nv,
                                                            (unsigned)(C / V),
                                                            make_fastdiv((unsigned)(rps * (C / V))));
  DCNN_LAUNCH_CHECK();
}

template <typename T>
void lscale_drop_bwd_t(const void* dy, const void* x, const float* gamma, const float* mask, void* dx, float* dgamma,
                       long R, int C, long rps, float* workspace, hipStream_t s) {
  const int dt = std::is_same<T, bf16>::value ? 1 : 0;
  const int grid = ln_partial_rows(R, C);
  ln_dispatch<T>(ln_shape(dt, C), [&](auto vpl, auto g) {
    lscale_drop_bwd_kernel<T, decltype(vpl)::value, decltype(g)::value><<<dim3(grid), dim3(256), 0, s>>>(
        (const T*)dy, (const T*)x, gamma, mask, (T*)dx, (int)R, C, make_fastdiv((unsigned)rps), workspace);
  });
  DCNN_LAUNCH_CHECK();
  ln_slab_reduce(workspace, grid, 1, C, dgamma, nullptr, s);
}

void lscale_drop_check(const char* what, int dt, long R, int C, long rps) {
  ln_check(what, dt, R, C);
  if (rps < 1 || R % rps)
    throw std::invalid_argument(std::string(what) + ": R=" + std::to_string(R) + " rows are not whole samples of " +
                                std::to_string(rps) + " rows");
}

}  // namespace lnorm
using namespace lnorm;

bool ln_supported(int dt, long R, int C) {
  if (dt != 0 && dt != 1) return false;
  return R >= 1 && C >= 8 && C <= 2048 && C % (dt == 1 ? 8 : 4) == 0 && R * (long)C < (1l << 31);
}

// The same for both dtypes: the bf16 lane group is the narrower one, so this many workgroups
// each own at least one row group in the fp32 instance too.
int ln_partial_rows(long R, int C) {
  if (R < 1 || C < 8 || C > 2048) return 0;
  return std::min(ln_groups(1, R, C - C % 8), kLnBwdGridCap);
}

long ln_workspace_bytes(long R, int C) { return (long)ln_partial_rows(R, C) * 2 * C * (long)sizeof(float); }

void ln_fwd(int dt, const void* x, void* y, long R, int C, const float* gamma, const float* beta, float eps,
            float* save_mean, float* save_rstd, hipStream_t s) {
  ln_check("ln_fwd", dt, R, C);
  if (dt == 1) ln_fwd_t<bf16>(x, y, R, C, gamma, beta, eps, save_mean, save_rstd, s);
  else ln_fwd_t<float>(x, y, R, C, gamma, beta, eps, save_mean, save_rstd, s);
}

void ln_bwd(int dt, const void* dy, const void* x, void* dx, long R, int C, const float* gamma, const float* mean,
            const float* rstd, float* dgamma, float* dbeta, float* workspace, hipStream_t s) {
  ln_check("ln_bwd", dt, R, C);
  if ((dgamma || dbeta) && !workspace) throw std::invalid_argument("ln_bwd: affine gradients need a workspace");
  if (dt == 1) ln_bwd_t<bf16>(dy, x, dx, R, C, gamma, mean, rstd, dgamma, dbeta, workspace, s);
  else ln_bwd_t<float>(dy, x, dx, R, C, gamma, mean, rstd, dgamma, dbeta, workspace, s);
}

void lscale_fwd(int dt, const void* x, const float* gamma, const void* residual, void* y, long R, int C,
                hipStream_t s) {
  ln_check("lscale_fwd", dt, R, C);
  if (dt == 1) lscale_fwd_t<bf16>(x, gamma, residual, y, R, C, s);
  else lscale_fwd_t<float>(x, gamma, residual, y, R, C, s);
}

void lscale_bwd(int dt, const void* dy, const void* x, const float* gamma, void* dx, float* dgamma, long R, int C,
                float* workspace, hipStream_t s) {
  ln_check("lscale_bwd", dt, R, C);
  if (!dgamma || !workspace) throw std::invalid_argument("lscale_bwd: needs dgamma and a workspace");
  if (dt == 1) lscale_bwd_t<bf16>(dy, x, gamma, dx, dgamma, R, C, workspace, s);
  else lscale_bwd_t<float>(dy, x, gamma, dx, dgamma, R, C, workspace, s);
}

void lscale_drop_fwd(int dt, const void* x, const float* gamma, const float* mask, const void* residual, void* y,
                     long R, int C, long rows_per_sample, hipStream_t s) {
  lscale_drop_check("lscale_drop_fwd", dt, R, C, rows_per_sample);
  if (!mask || !residual) throw std::invalid_argument("lscale_drop_fwd: needs a mask and a residual");
  if (dt == 1) lscale_drop_fwd_t<bf16>(x, gamma, mask, residual, y, R, C, rows_per_sample, s);
  else lscale_drop_fwd_t<float>(x, gamma, mask, residual, y, R, C, rows_per_sample, s);
}

void lscale_drop_bwd(int dt, const void* dy, const void* x, const float* gamma, const float* mask, void* dx,
                     float* dgamma, long R, int C, long rows_per_sample, float* workspace, hipStream_t s) {
  lscale_drop_check("lscale_drop_bwd", dt, R, C, rows_per_sample);
  if (!mask || !dgamma || !workspace) throw std::invalid_argument("lscale_drop_bwd: needs a mask, dgamma and a workspace");
  if (dt == 1) lscale_drop_bwd_t<bf16>(dy, x, gamma, mask, dx, dgamma, R, C, rows_per_sample, workspace, s);
  else lscale_drop_bwd_t<float>(dy, x, gamma, mask, dx, dgamma, R, C, rows_per_sample, workspace, s);
}

}  // namespace dcnn
