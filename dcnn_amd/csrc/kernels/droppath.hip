// Stochastic depth (DropPath): the per-sample mask and the standalone per-sample scale.
//
// The mask is one function of (seed, draw, n), the same on every device and in both front ends
// (the native CPU copy is cpu_ops.cpp drop_path_mask): Philox-4x32-10 with the key
// seed + draw * 0x9E3779B97F4A7C15, counter n / 4, lane n % 4; sample n is kept when u01 >= p and
// then scaled by 1 / (1 - p). The keep scale is computed on the host (drop_path_keep_scale) so every
// backend multiplies by the same bits. No reference counterpart (the reference has no such layer).
//
// drop_path_mask_kernel writes the N floats once per training forward; the draw index comes from a
// device word written by counter_bump (pool_act.hip), so a replayed hipGraph draws a new mask at
// every replay. drop_path_scale_kernel is forward and backward alike: y[n] = m[n] x[n] (+ res[n]).
// A sample is `row` contiguous elements; each sample's span is split into a scalar head up to the
// next 16-byte boundary, 16-byte vectors, and a scalar tail, so any row length works and no
// vector straddles two samples. A dropped sample's span is written without reading x. The fused
// form (the mask inside a LayerScale's residual store) is lscale_drop_fwd / _bwd in lnorm.hip.
#include <algorithm>
#include <stdexcept>
#include <string>

#include "common.h"
#include "api.h"

namespace dcnn {
namespace droppath {

__global__ void drop_path_mask_kernel(float* __restrict__ mask, int N, float p, float keep_scale, uint64_t seed,
                                      uint64_t draw, const uint64_t* __restrict__ ctr) {
  if (ctr) draw = *ctr;
  const uint64_t key = seed + draw * 0x9E3779B97F4A7C15ull;
  const int nq = (N + 3) / 4;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += gridDim.x * blockDim.x) {
    const uint4 r = Philox::gen(key, (uint64_t)q);
    const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int n = q * 4 + v;
      if (n < N) mask[n] = Philox::u01(rr[v]) >= p ? keep_scale : 0.f;
    }
  }
}

template <typename T>
struct DpVec;
template <>
struct DpVec<bf16> {
  static constexpr int V = 8;
  __device__ static __forceinline__ void load(const bf16* p, float* f) { unpack8(*reinterpret_cast<const uint4*>(p), f); }
  __device__ static __forceinline__ void store(bf16* p, const float* f) { *reinterpret_cast<uint4*>(p) = pack8(f); }
};
template <>
struct DpVec<float> {
  static constexpr int V = 4;
  __device__ static __forceinline__ void load(const float* p, float* f) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  }
  __device__ static __forceinline__ void store(float* p, const float* f) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  }
};

// y[n][:] = mask[n] x[n][:] (+ res[n][:]); blockIdx.y walks the samples, blockIdx.x the span.
// x, y and res share their address modulo 16 (checked by the launcher).
template <typename T, bool RES>
__global__ void __launch_bounds__(256) drop_path_scale_kernel(const T* __restrict__ x, const float* __restrict__ mask,
                                                              const T* __restrict__ res, T* __restrict__ y, long N,
                                                              long row) {
  constexpr int V = DpVec<T>::V;
  for (long n = blockIdx.y; n < N; n += gridDim.y) {
    const float m = mask[n];
    const long base = n * row;
    const long mis = (long)(((uintptr_t)(y + base) & 15) / sizeof(T));  // elements past a 16-byte boundary
    const long head = std::min(row, (V - mis) % V);
    const long nvec = (row - head) / V;
    const long tail0 = head + nvec * V;
    for (long i = blockIdx.x * 256l + threadIdx.x; i < nvec; i += gridDim.x * 256l) {
      const long o = base + head + i * V;
      float f[V];
      if (m != 0.f) {
        DpVec<T>::load(x + o, f);
#pragma unroll
        for (int v = 0; v < V; ++v) f[v] *= m;
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) f[v] = 0.f;
      }
      if (RES) {
        float r[V];
        DpVec<T>::load(res + o, r);
#pragma unroll
        for (int v = 0; v < V; ++v) f[v] += r[v];
      }
      DpVec<T>::store(y + o, f);
    }
    if (blockIdx.x == 0) {  // the scalar head and tail of this sample's span
      const long ns = head + (row - tail0);
      for (long e = threadIdx.x; e < ns; e += 256) {
        const long o = base + (e < head ? e : tail0 + (e - head));
        float f = m != 0.f ? to_f(x[o]) * m : 0.f;
        if (RES) f += to_f(res[o]);
        y[o] = from_f<T>(f);
      }
    }
  }
}

template <typename T>
void scale_t(const void* x, const float* mask, const void* res, void* y, long N, long row, hipStream_t s) {
  constexpr int V = DpVec<T>::V;
  const dim3 grid(grid_for(row / V + 1, 256, 1024), (unsigned)std::min(N, 4096l));
  if (res)
    drop_path_scale_kernel<T, true><<<grid, dim3(256), 0, s>>>((const T*)x, mask, (const T*)res, (T*)y, N, row);
  else
    drop_path_scale_kernel<T, false><<<grid, dim3(256), 0, s>>>((const T*)x, mask, nullptr, (T*)y, N, row);
  DCNN_LAUNCH_CHECK();
}

}  // namespace droppath

float drop_path_keep_scale(float p) {
  if (!(p >= 0.f && p < 1.f)) throw std::invalid_argument("drop_path: rate " + std::to_string(p) + " is not in [0, 1)");
  return 1.0f / (1.0f - p);
}

void drop_path_mask(float* mask, int N, float p, uint64_t seed, uint64_t draw, const uint64_t* ctr, hipStream_t s) {
  const float ks = drop_path_keep_scale(p);
  if (N < 1) throw std::invalid_argument("drop_path_mask: N=" + std::to_string(N) + " samples");
  droppath::drop_path_mask_kernel<<<dim3(grid_for((N + 3) / 4, 64, 1024)), dim3(64), 0, s>>>(mask, N, p, ks, seed, draw,
                                                                                            ctr);
  DCNN_LAUNCH_CHECK();
}

void drop_path_scale(int dt, const void* x, const float* mask, const void* residual, void* y, long N, long row,
                     hipStream_t s) {
  if ((dt != 0 && dt != 1) || N < 1 || row < 1)
    throw std::invalid_argument("drop_path_scale: unsupported shape: N=" + std::to_string(N) + " samples of " +
                                std::to_string(row) + " elements, dtype code " + std::to_string(dt));
  const uintptr_t es = dt == 1 ? 2 : 4, a = (uintptr_t)y;
  if (a % es || ((uintptr_t)x ^ a) & 15 || (residual && ((uintptr_t)residual ^ a) & 15))
    throw std::invalid_argument("drop_path_scale: x, y and the residual must share their address modulo 16");
  if (dt == 1) droppath::scale_t<bf16>(x, mask, residual, y, N, row, s);
  else droppath::scale_t<float>(x, mask, residual, y, N, row, s);
}

}  // namespace dcnn
