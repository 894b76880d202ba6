// Layer-wise adaptive optimizers over the flat parameter arena: LAMB (Adam with a per-parameter
// trust ratio) and LARS (momentum SGD with one), You et al. 2017 / 2019.
//
// What sets them apart from adam_kernel / sgd_kernel is one L2 norm PER PARAMETER of the weights and
// of the update. The arena stays flat and the step stays inside a captured graph: a step is two
// launches driven by the static chunk table of optim_segments.h.
//   pass 1 (lamb_moments_kernel / lars_norms_kernel): a workgroup takes chunks c = blockIdx.x,
//     + gridDim.x, ...; each chunk's {sum p^2, sum u^2} is a fixed tree over that chunk's elements,
//     stored as one partial pair per chunk. The workgroups then take the self-resetting ticket that
//     grad_sumsq_kernel and loss_kernel use, and the last one adds every segment's partials in a
//     fixed order over the chunk index and writes trust[segment]. No float atomics; the result
//     depends on the table only, never on the grid, so eager and replayed steps agree bit for bit.
//   pass 2 (lamb_apply_kernel / lars_apply_kernel): per chunk again, reads trust[segment] and applies
//     the step, the EMA and the bf16 shadow refresh as the tail kernels of loss_optim.hip do.
// LAMB does not store its update r: pass 2 recomputes it from the new m, v and the old p with the one
// __device__ function pass 1 used (lamb_r), which costs 3 reads there instead of a fifth buffer.
// Chunks are 64-element aligned (the arena's slice alignment) and at most 4096 elements; the gaps
// between slices are zero in every buffer and stay zero under both steps.
#include "common.h"
#include "api.h"

namespace dcnn {

constexpr int kLwLanes = 1024;     // pass 1: one float4 of a full chunk per lane
constexpr int kLwWaves = kLwLanes / 64;
constexpr int kLwApplyLanes = 256; // pass 2: four float4 of a full chunk per lane
static_assert(kSegChunkBlocks * kSegBlock == kLwLanes * 4 && kSegPartFloats == 2,
              "a full chunk is one float4 per pass-1 lane; one partial pair per chunk");
static_assert(kSegChunkBlocks * kSegBlock == kLwApplyLanes * 16, "a full chunk is four float4 per pass-2 lane");

// r = (m / bc1) / (sqrt(v / bc2) + eps) + wd p with every rounding spelled out (no contraction), so
// that pass 1 and pass 2 form identical bits from identical inputs.
__device__ __forceinline__ float lamb_r(float p, float m, float v, float bc1, float bc2, float eps, float wd) {
#pragma clang fp contract(off)
  const float mh = m / bc1, vh = v / bc2;
  const float den = sqrtf(vh) + eps;
  const float q = mh / den, d = wd * p;
  return q + d;
}

__device__ __forceinline__ float sq4(const float4 x) {
#pragma clang fp contract(off)
  const float a = x.x * x.x, b = x.y * x.y, c = x.z * x.z, d = x.w * x.w;
  return (a + b) + (c + d);
}

// The chunk's pair from the lanes' values: wave butterflies, then the sixteen wave sums pairwise (wave
// 0 for the first component, wave 1 for the second). sw is indexed by the loop's parity, so one
// barrier per chunk is enough: a slot is rewritten two barriers after it was read.
__device__ __forceinline__ void lw_chunk_pair(float a, float b, float (*sw)[2][kLwWaves], int par, float* part, int c) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane == 0) {
    sw[par][0][w] = a;
    sw[par][1][w] = b;
  }
  __syncthreads();
  if (lane == 0 && w < 2) {
    float t[kLwWaves];
#pragma unroll
    for (int i = 0; i < kLwWaves; ++i) t[i] = sw[par][w][i];
#pragma unroll
    for (int o = kLwWaves / 2; o > 0; o >>= 1)
#pragma unroll
      for (int i = 0; i < o; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    part[2 * (long)c + w] = t[0];
  }
}

// The ticket of grad_sumsq_kernel (agent release before it, agent acquire behind it in the last
// workgroup), then the last workgroup's finishing step: wave w takes segments w, w + 16, ...; its lane
// l adds the partials of chunks l, l + 64, ... of the segment in order, then a wave butterfly. More
// segments than lanes or waves are simply more turns of the loop. out: trust [nsegs], then the pairs
// {sum p^2, sum u^2} [nsegs][2]. trust_of(sum p^2, sum u^2, decay) is called for adapting segments.
template <typename F>
__device__ __forceinline__ void lw_finish(float* part, unsigned* __restrict__ ticket,
                                          const SegInfo* __restrict__ segs, int nsegs, float* __restrict__ out,
                                          F trust_of) {
  __shared__ int last;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0 && w < 2) {  // the two lanes that stored partials drain their stores
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = old == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  for (int s = w; s < nsegs; s += kLwWaves) {
    const SegInfo g = segs[s];
    float a = 0.f, b = 0.f;
    for (int k = lane; k < g.chunks; k += 64) {
      const float2 x = reinterpret_cast<const float2*>(part)[g.first_chunk + k];
      a += x.x;
      b += x.y;
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
      out[s] = g.adapt ? trust_of(a, b, g.decay) : 1.f;
      out[nsegs + 2 * (long)s] = a;
      out[nsegs + 2 * (long)s + 1] = b;
    }
  }
  if (threadIdx.x == 0) *ticket = 0u;  // ready for the next step on this stream
}

// ------------------------------------------------------------------------------------------- LAMB
// The step scalars on the device, as adam_scalars keeps them (hyper = {lr, bc1, bc2, t}: t += 1, the
// bias corrections of the new t), but from the betas in double: 1 - float(0.999) is 4.7e-5 off 0.001.
// In an Adam update that error cancels between the second moment and its correction; the moment
// itself, which LAMB's state is compared by, carries it. The moments kernel takes 1 - beta rounded
// from double for the same reason.
__global__ void lamb_scalars_kernel(float* hyper, double b1, double b2) {
  if (threadIdx.x == 0) {
    const float t = hyper[3] + 1.f;
    hyper[3] = t;
    hyper[1] = (float)(1.0 - pow(b1, (double)t));
    hyper[2] = (float)(1.0 - pow(b2, (double)t));
  }
}

void lamb_scalars(float* hyper, double b1, double b2, hipStream_t s) {
  hipLaunchKernelGGL(lamb_scalars_kernel, dim3(1), dim3(64), 0, s, hyper, b1, b2);
  DCNN_LAUNCH_CHECK();
}

// Pass 1: m, v updated in place, r formed in registers, {sum p^2, sum r^2} per chunk, trust per segment.
// trust = ||p|| / ||r|| where the segment adapts and neither norm is zero, else 1; a NaN norm is not
// zero, so it propagates into the step (no step is skipped, as with clipping).
__global__ void __launch_bounds__(kLwLanes)
lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                    float* __restrict__ v, float b1, float b2, float k1, float k2, float eps, float bc1, float bc2,
                    float wd, const float* __restrict__ hyper, const float* __restrict__ coef,
                    const SegChunk* __restrict__ chunks, int nchunks, const SegInfo* __restrict__ segs, int nsegs,
                    float* part, unsigned* __restrict__ ticket, float* __restrict__ out) {
  __shared__ float sw[2][2][kLwWaves];
  if (hyper) { bc1 = hyper[1]; bc2 = hyper[2]; }
  const float c = coef ? *coef : 1.f;
  int par = 0;
  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x, par ^= 1) {
    const SegChunk k = chunks[ch];
    const float w = segs[k.segment].decay ? wd : 0.f;
    float a = 0.f, b = 0.f;
    if ((int)threadIdx.x < k.blocks * 16) {
      const long i = (long)k.first_block * 16 + threadIdx.x;
      const float4 pp = reinterpret_cast<const float4*>(p)[i];
      float4 gg = reinterpret_cast<const float4*>(g)[i];
      float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
      if (coef) { gg.x *= c; gg.y *= c; gg.z *= c; gg.w *= c; }
      mm.x = b1 * mm.x + k1 * gg.x; vv.x = b2 * vv.x + k2 * gg.x * gg.x;
      mm.y = b1 * mm.y + k1 * gg.y; vv.y = b2 * vv.y + k2 * gg.y * gg.y;
      mm.z = b1 * mm.z + k1 * gg.z; vv.z = b2 * vv.z + k2 * gg.z * gg.z;
      mm.w = b1 * mm.w + k1 * gg.w; vv.w = b2 * vv.w + k2 * gg.w * gg.w;
      reinterpret_cast<float4*>(m)[i] = mm;
      reinterpret_cast<float4*>(v)[i] = vv;
      const float4 r = {lamb_r(pp.x, mm.x, vv.x, bc1, bc2, eps, w), lamb_r(pp.y, mm.y, vv.y, bc1, bc2, eps, w),
                        lamb_r(pp.z, mm.z, vv.z, bc1, bc2, eps, w), lamb_r(pp.w, mm.w, vv.w, bc1, bc2, eps, w)};
      a = sq4(pp);
      b = sq4(r);
    }
    lw_chunk_pair(a, b, sw, par, part, ch);
  }
  lw_finish(part, ticket, segs, nsegs, out, [](float sp, float sr, int) {
    const float pn = sqrtf(sp), rn = sqrtf(sr);
    return (pn == 0.f || rn == 0.f) ? 1.f : pn / rn;
  });
}

// Pass 2: p -= lr trust[segment] r, r recomputed from the old p and the new m, v; EMA and shadow as
// in adam_tail_kernel.
__global__ void __launch_bounds__(kLwApplyLanes)
lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                  bf16* __restrict__ shadow, float lr, float eps, float bc1, float bc2, float wd,
                  const float* __restrict__ hyper, float* __restrict__ ema, float decay,
                  const SegChunk* __restrict__ chunks, int nchunks, const SegInfo* __restrict__ segs,
                  const float* __restrict__ trust) {
  if (hyper) { lr = hyper[0]; bc1 = hyper[1]; bc2 = hyper[2]; }
  const float keep = 1.f - decay;
  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const SegChunk k = chunks[ch];
    const float w = segs[k.segment].decay ? wd : 0.f, s = lr * trust[k.segment];
    const long base = (long)k.first_block * 16;
    const int n4 = k.blocks * 16;
    float4 pp[4], mm[4], vv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = j * kLwApplyLanes + threadIdx.x;
      if (t < n4) {
        pp[j] = reinterpret_cast<float4*>(p)[base + t];
        mm[j] = reinterpret_cast<const float4*>(m)[base + t];
        vv[j] = reinterpret_cast<const float4*>(v)[base + t];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = j * kLwApplyLanes + threadIdx.x;
      if (t >= n4) continue;
      float4 q = pp[j];
      q.x = __fmaf_rn(-s, lamb_r(q.x, mm[j].x, vv[j].x, bc1, bc2, eps, w), q.x);
      q.y = __fmaf_rn(-s, lamb_r(q.y, mm[j].y, vv[j].y, bc1, bc2, eps, w), q.y);
      q.z = __fmaf_rn(-s, lamb_r(q.z, mm[j].z, vv[j].z, bc1, bc2, eps, w), q.z);
      q.w = __fmaf_rn(-s, lamb_r(q.w, mm[j].w, vv[j].w, bc1, bc2, eps, w), q.w);
      reinterpret_cast<float4*>(p)[base + t] = q;
      if (ema) {
        float4 e = reinterpret_cast<float4*>(ema)[base + t];
        e.x = __fmaf_rn(decay, e.x, keep * q.x);
        e.y = __fmaf_rn(decay, e.y, keep * q.y);
        e.z = __fmaf_rn(decay, e.z, keep * q.z);
        e.w = __fmaf_rn(decay, e.w, keep * q.w);
        reinterpret_cast<float4*>(ema)[base + t] = e;
      }
      if (shadow) {
        bf16x4 h = {(bf16)q.x, (bf16)q.y, (bf16)q.z, (bf16)q.w};
        reinterpret_cast<bf16x4*>(shadow)[base + t] = h;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- LARS
// Pass 1: {sum p^2, sum g^2} per chunk; trust = tc ||p|| / (coef ||g|| + wd_i ||p|| + eps) where the
// segment adapts and neither norm is zero, else 1 (a NaN norm propagates).
__global__ void __launch_bounds__(kLwLanes)
lars_norms_kernel(const float* __restrict__ p, const float* __restrict__ g, float wd, float tc, float eps,
                  const float* __restrict__ coef, const SegChunk* __restrict__ chunks, int nchunks,
                  const SegInfo* __restrict__ segs, int nsegs, float* part, unsigned* __restrict__ ticket,
                  float* __restrict__ out) {
  __shared__ float sw[2][2][kLwWaves];
  int par = 0;
  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x, par ^= 1) {
    const SegChunk k = chunks[ch];
    float a = 0.f, b = 0.f;
    if ((int)threadIdx.x < k.blocks * 16) {
      const long i = (long)k.first_block * 16 + threadIdx.x;
      a = sq4(reinterpret_cast<const float4*>(p)[i]);
      b = sq4(reinterpret_cast<const float4*>(g)[i]);
    }
    lw_chunk_pair(a, b, sw, par, part, ch);
  }
  const float c = coef ? *coef : 1.f;
  lw_finish(part, ticket, segs, nsegs, out, [=](float sp, float sg, int decay) {
    const float pn = sqrtf(sp), gn = c * sqrtf(sg);
    return (pn == 0.f || gn == 0.f) ? 1.f : tc * pn / (gn + (decay ? wd : 0.f) * pn + eps);
  });
}

// v = mom v - s (g + wd_i p), p += v, or p -= s (g + wd_i p) without a velocity, s = lr trust: the
// roundings spelled out as in sgd1.
__device__ __forceinline__ float lars1(float& p, float g, float& vel, bool has_vel, float s, float mom, float wd) {
#pragma clang fp contract(off)
  const float d = wd * p;
  const float u = g + d;
  if (has_vel) {
    const float a = mom * vel, b = s * u;
    const float vv = a - b;
    vel = vv;
    p += vv;
  } else {
    p = __fmaf_rn(-s, u, p);
  }
  return p;
}

// Pass 2: sgd_tail_kernel's body with trust[segment] and wd_i.
__global__ void __launch_bounds__(kLwApplyLanes)
lars_apply_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ vel,
                  bf16* __restrict__ shadow, float lr, float mom, float wd, const float* __restrict__ hyper,
                  const float* __restrict__ coef, float* __restrict__ ema, float decay,
                  const SegChunk* __restrict__ chunks, int nchunks, const SegInfo* __restrict__ segs,
                  const float* __restrict__ trust) {
  if (hyper) lr = hyper[0];
  const float c = coef ? *coef : 1.f, keep = 1.f - decay;
  const bool hv = vel != nullptr;
  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const SegChunk k = chunks[ch];
    const float w = segs[k.segment].decay ? wd : 0.f, s = lr * trust[k.segment];
    const long base = (long)k.first_block * 16;
    const int n4 = k.blocks * 16;
    float4 pp[4], gg[4], vv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = j * kLwApplyLanes + threadIdx.x;
      vv[j] = float4{0.f, 0.f, 0.f, 0.f};
      if (t < n4) {
        pp[j] = reinterpret_cast<float4*>(p)[base + t];
        gg[j] = reinterpret_cast<const float4*>(g)[base + t];
        if (hv) vv[j] = reinterpret_cast<float4*>(vel)[base + t];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = j * kLwApplyLanes + threadIdx.x;
      if (t >= n4) continue;
      float4 q = pp[j], x = gg[j], y = vv[j];
      if (coef) { x.x *= c; x.y *= c; x.z *= c; x.w *= c; }
      lars1(q.x, x.x, y.x, hv, s, mom, w);
      lars1(q.y, x.y, y.y, hv, s, mom, w);
      lars1(q.z, x.z, y.z, hv, s, mom, w);
      lars1(q.w, x.w, y.w, hv, s, mom, w);
      reinterpret_cast<float4*>(p)[base + t] = q;
      if (hv) reinterpret_cast<float4*>(vel)[base + t] = y;
      if (ema) {
        float4 e = reinterpret_cast<float4*>(ema)[base + t];
        e.x = __fmaf_rn(decay, e.x, keep * q.x);
        e.y = __fmaf_rn(decay, e.y, keep * q.y);
        e.z = __fmaf_rn(decay, e.z, keep * q.z);
        e.w = __fmaf_rn(decay, e.w, keep * q.w);
        reinterpret_cast<float4*>(ema)[base + t] = e;
      }
      if (shadow) {
        bf16x4 h = {(bf16)q.x, (bf16)q.y, (bf16)q.z, (bf16)q.w};
        reinterpret_cast<bf16x4*>(shadow)[base + t] = h;
      }
    }
  }
}

// -------------------------------------------------------------------------------------- launchers
static void lw_check(const char* who, const void* p, const void* g, long n, const LayerwiseTables& t, const float* ema,
                     float decay) {
  const std::string w(who);
  if (n < 1 || !p || !g) throw std::invalid_argument(w + ": p, g and n >= 1 are required");
  if (((uintptr_t)p & 15) || ((uintptr_t)g & 15)) throw std::invalid_argument(w + ": the buffers are 16-byte aligned");
  if (t.nchunks < 0 || t.nsegs < 0 || (t.nchunks && !t.chunks) || (t.nsegs && !t.segs))
    throw std::invalid_argument(w + ": the chunk table (" + std::to_string(t.nchunks) + " rows) or the segment table (" +
                                std::to_string(t.nsegs) + " rows) is missing");
  if (t.cover > n || t.cover % kSegBlock != 0)
    throw std::invalid_argument(w + ": the chunk table reaches element " + std::to_string(t.cover) +
                                ", the buffers hold " + std::to_string(n) + "; every chunk is a whole number of " +
                                std::to_string(kSegBlock) + "-element blocks inside the buffers");
  if (!t.part || !t.ticket || !t.out)
    throw std::invalid_argument(w + ": partials [2 x chunks], the ticket word and the trust table [3 x segments] are required");
  if (ema && !(decay > 0.f && decay < 1.f))
    throw std::invalid_argument(w + ": ema_decay " + std::to_string(decay) + " is not in (0, 1)");
}

// a function of the table alone (and the result does not depend on it)
static int lw_norm_grid(int nchunks) { return nchunks < 1 ? 1 : nchunks > 512 ? 512 : nchunks; }
static int lw_apply_grid(int nchunks) { return nchunks < 1 ? 1 : nchunks > 4096 ? 4096 : nchunks; }

void lamb_step(float* p, const float* g, float* m, float* v, bf16* shadow, long n, float lr, double b1, double b2,
               float eps, float bc1, float bc2, float wd, const float* hyper, const float* coef, float* ema,
               float decay, const LayerwiseTables& t, hipStream_t s) {
  lw_check("lamb_step", p, g, n, t, ema, decay);
  if (!m || !v) throw std::invalid_argument("lamb_step: m and v are required");
  if (t.nsegs == 0) return;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(lw_norm_grid(t.nchunks)), dim3(kLwLanes), 0, s, p, g, m, v, (float)b1,
                     (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), eps, bc1, bc2, wd, hyper, coef, t.chunks, t.nchunks, t.segs, t.nsegs, t.part, t.ticket, t.out);
  DCNN_LAUNCH_CHECK();
  if (t.nchunks == 0) return;
  hipLaunchKernelGGL(lamb_apply_kernel, dim3(lw_apply_grid(t.nchunks)), dim3(kLwApplyLanes), 0, s, p, m, v, shadow, lr,
                     eps, bc1, bc2, wd, hyper, ema, decay, t.chunks, t.nchunks, t.segs, t.out);
  DCNN_LAUNCH_CHECK();
}

void lars_step(float* p, const float* g, float* vel, bf16* shadow, long n, float lr, float mom, float wd, float tc,
               float eps, const float* hyper, const float* coef, float* ema, float decay, const LayerwiseTables& t,
               hipStream_t s) {
  lw_check("lars_step", p, g, n, t, ema, decay);
  if (t.nsegs == 0) return;
  hipLaunchKernelGGL(lars_norms_kernel, dim3(lw_norm_grid(t.nchunks)), dim3(kLwLanes), 0, s, p, g, wd, tc, eps, coef,
                     t.chunks, t.nchunks, t.segs, t.nsegs, t.part, t.ticket, t.out);
  DCNN_LAUNCH_CHECK();
  if (t.nchunks == 0) return;
  hipLaunchKernelGGL(lars_apply_kernel, dim3(lw_apply_grid(t.nchunks)), dim3(kLwApplyLanes), 0, s, p, g, vel, shadow, lr,
                     mom, wd, hyper, coef, ema, decay, t.chunks, t.nchunks, t.segs, t.out);
  DCNN_LAUNCH_CHECK();
}

}  // namespace dcnn
