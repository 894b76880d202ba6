// Fused loss (+gradient +accuracy) and flat-buffer optimizer kernels.
//
// Reference: K37/K38 (src/nn/loss_impl/cuda/loss_ops.cu:18-376: separate loss / grad kernels,
// cudaMallocAsync + two-stage reduce + D2H + stream sync per call), K41 accuracy
// (src/utils/accuracy_impl/cuda/accuracy.cu:15-115: cudaMalloc per call, default stream),
// K39/K40 Adam/SGD (one launch PER parameter tensor).
// Here: ONE kernel computes loss, gradient and the correct-count per batch (one wave per
// sample row, device-side scalars, no host sync, graph-capturable); optimizers run ONE
// launch over the flat fp32 master buffer and refresh the bf16 shadow copy used by the
// MFMA kernels in the same pass.
#include "common.h"
#include "api.h"

namespace dcnn {

enum LossType { kCE = 0, kSoftmaxCE = 1, kLogSoftmaxCE = 2, kMSE = 3, kMAE = 4, kHuber = 5, kSoftCE = 6 };

// One wave per sample row (4 rows per workgroup). Each row's loss and hit are written to a
// workspace; the workgroups then take a ticket and the last one sums the N row values in a
// fixed pairwise order (agent release / acquire around the ticket): the loss is bit-reproducible
// with no float atomics and no memset of the outputs.
template <typename T>
__device__ __forceinline__ void loss_row(const T* __restrict__ pred, const float* __restrict__ target,
                                         const int64_t* __restrict__ labels, T* __restrict__ grad, int row, int N,
                                         int C, int type, float param, float gscale, int lane, float* lsum_out,
                                         int* hit) {
  const T* p = pred + (long)row * C;
  auto tgt = [&](int c) -> float {
    if (labels) return (int64_t)c == labels[row] ? 1.f : 0.f;
    return target[(long)row * C + c];
  };
  // argmax of prediction and of target (first max wins)
  float pm = -INFINITY, tm = -INFINITY;
  int pi = 0x7fffffff, ti = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = to_f(p[c]), t = tgt(c);
    if (v > pm) { pm = v; pi = c; }
    if (t > tm) { tm = t; ti = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float pv = __shfl_xor(pm, o, 64), tv = __shfl_xor(tm, o, 64);
    const int pj = __shfl_xor(pi, o, 64), tj = __shfl_xor(ti, o, 64);
    if (pv > pm || (pv == pm && pj < pi)) { pm = pv; pi = pj; }
    if (tv > tm || (tv == tm && tj < ti)) { tm = tv; ti = tj; }
  }
  const float invN = 1.f / (float)N, invNC = 1.f / ((float)N * (float)C);
  // gradient scale: gscale = 1 / world under data parallelism (the gradient average folded into
  // the loss gradient, so no separate pass scales it)
  const float ginvN = invN * gscale, ginvNC = invNC * gscale;
  float lsum = 0.f;
  if (type == kSoftmaxCE || type == kLogSoftmaxCE) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += __expf(to_f(p[c]) - pm);
    s = wave_sum(s);
    const float lse = pm + __logf(s);
    // loss uses the first class whose target > 0.5 (loss_ops.cpp semantics)
    int hot = 0x7fffffff;
    for (int c = lane; c < C; c += 64) if (tgt(c) > 0.5f && c < hot) hot = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hot = min(hot, __shfl_xor(hot, o, 64));
    if (hot < C) lsum = (lse - to_f(p[hot])) * invN;
    if (grad) {
      const float inv_s = 1.f / s;
      for (int c = lane; c < C; c += 64)
        grad[(long)row * C + c] = from_f<T>((__expf(to_f(p[c]) - pm) * inv_s - tgt(c)) * ginvN);
    }
  } else if (type == kSoftCE) {
    // soft-target CE with label smoothing (param = eps): t' = (1 - eps) t + eps / C, S = sum t',
    // loss = S lse - sum t' x, grad = S softmax - t'. No hot class: any dense target is valid.
    const float keep = 1.f - param, fl = param / (float)C;
    float s = 0.f, S = 0.f, dot = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float v = to_f(p[c]), ts = __fmaf_rn(keep, tgt(c), fl);
      s += __expf(v - pm);
      S += ts;
      dot = __fmaf_rn(ts, v, dot);
    }
    s = wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // S and sum t' x in one pass over the wave
      S += __shfl_xor(S, o, 64);
      dot += __shfl_xor(dot, o, 64);
    }
    const float lse = pm + __logf(s);
    lsum = (S * lse - dot) * invN;
    if (grad) {
      const float Sinv_s = S / s;
      for (int c = lane; c < C; c += 64)
        grad[(long)row * C + c] =
            from_f<T>((__expf(to_f(p[c]) - pm) * Sinv_s - __fmaf_rn(keep, tgt(c), fl)) * ginvN);
    }
  } else if (type == kCE) {
    int hot = 0x7fffffff;
    for (int c = lane; c < C; c += 64) if (tgt(c) > 0.5f && c < hot) hot = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hot = min(hot, __shfl_xor(hot, o, 64));
    if (hot < C) {
      const float v = fminf(fmaxf(to_f(p[hot]), param), 1.f - param);
      lsum = -__logf(v) * invN;
    }
    if (grad)
      for (int c = lane; c < C; c += 64)
        grad[(long)row * C + c] = from_f<T>((to_f(p[c]) - tgt(c)) * ginvN);
  } else {
    for (int c = lane; c < C; c += 64) {
      const float d = to_f(p[c]) - tgt(c), ad = fabsf(d);
      float l, g;
      if (type == kMSE) { l = d * d; g = 2.f * d * ginvNC; }
      else if (type == kMAE) { l = ad; g = d > 0.f ? ginvNC : -ginvNC; }
      else {
        if (ad <= param) { l = 0.5f * d * d; g = d * ginvNC; }
        else { l = param * ad - 0.5f * param * param; g = (d > 0.f ? param : -param) * ginvNC; }
      }
      lsum += l;
      if (grad) grad[(long)row * C + c] = from_f<T>(g);
    }
    lsum = wave_sum(lsum) * invNC;
  }
  *lsum_out += lsum;
  *hit += (pi == ti) ? 1 : 0;
}

template <typename T>
__global__ void __launch_bounds__(256) loss_kernel(const T* __restrict__ pred, const float* __restrict__ target,
                                                   const int64_t* __restrict__ labels, T* __restrict__ grad,
                                                   float* __restrict__ loss_out, int* __restrict__ correct, int N,
                                                   int C, int type, float param, float gscale,
                                                   float* __restrict__ rowv, unsigned* __restrict__ ticket) {
  __shared__ float sl[256];
  __shared__ int sc[256];
  __shared__ int last;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w;
  float lsum = 0.f;
  int hits = 0;
  if (row < N) loss_row<T>(pred, target, labels, grad, row, N, C, type, param, gscale, lane, &lsum, &hits);
  if (gridDim.x == 1) {
    if (lane == 0) { sl[w] = lsum; sc[w] = hits; }
    __syncthreads();
    if (threadIdx.x == 0) {
      *loss_out = (sl[0] + sl[1]) + (sl[2] + sl[3]);
      if (correct) *correct = sc[0] + sc[1] + sc[2] + sc[3];
    }
    return;
  }
  if (lane == 0 && row < N) {
    rowv[row] = lsum;
    reinterpret_cast<int*>(rowv + N)[row] = hits;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
  // last workgroup: thread t sums rows t, t + 256, ... in order, then a fixed LDS tree
  float l = 0.f;
  int h = 0;
  for (int r = threadIdx.x; r < N; r += 256) { l += rowv[r]; h += reinterpret_cast<const int*>(rowv + N)[r]; }
  sl[threadIdx.x] = l;
  sc[threadIdx.x] = h;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; sc[threadIdx.x] += sc[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *loss_out = sl[0];
    if (correct) *correct = sc[0];
    *ticket = 0u;  // ready for the next loss on this stream
  }
}

int loss_workspace_floats(int N) { return 2 * N; }

void loss_fused(int dt, const void* pred, const float* target, const int64_t* labels, void* grad, float* loss_out,
                int* correct, int N, int C, int type, float param, float gscale, float* ws, unsigned* ticket,
                hipStream_t s) {
  const int blocks = (N + 3) / 4;
  if (blocks > 1 && (!ws || !ticket)) throw std::runtime_error("loss_fused: workspace required");
  if (type < 0 || type > kSoftCE) throw std::invalid_argument("loss_fused: unknown loss kind " + std::to_string(type));
  if (type == kSoftCE && !(param >= 0.f && param < 1.f))
    throw std::invalid_argument("loss_fused: label_smoothing " + std::to_string(param) + " is not in [0, 1)");
  if (dt == 0)
    hipLaunchKernelGGL(loss_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)pred, target, labels,
                       (float*)grad, loss_out, correct, N, C, type, param, gscale, ws, ticket);
  else
    hipLaunchKernelGGL(loss_kernel<bf16>, dim3(blocks), dim3(256), 0, s, (const bf16*)pred, target, labels,
                       (bf16*)grad, loss_out, correct, N, C, type, param, gscale, ws, ticket);
  DCNN_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------
// Adam / AdamW over the flat master buffer (+ bf16 shadow refresh). Semantics of
// src/nn/optimizers_impl/cuda/adam_kernels.cu:17-57: bias-corrected, epsilon after sqrt,
// L2 variant adds wd*lr*param to the update, AdamW decays the parameter first.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float adam1(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps,
                                       float bc1, float bc2, float wd, int decoupled) {
  m = b1 * m + (1.f - b1) * g;
  v = b2 * v + (1.f - b2) * g * g;
  float upd = lr * (m / bc1) / (sqrtf(v / bc2) + eps);
  if (wd > 0.f) {
    if (decoupled) p -= wd * lr * p;
    else upd += wd * lr * p;
  }
  p -= upd;
  return p;
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, bf16* __restrict__ shadow, long n, float lr, float b1, float b2,
                            float eps, float bc1, float bc2, float wd, int decoupled,
                            const float* __restrict__ hyper) {
  // hyper (optional, device memory): {lr, bc1, bc2} so a captured hipGraph replays with the
  // current step's values without re-capture.
  if (hyper) { lr = hyper[0]; bc1 = hyper[1]; bc2 = hyper[2]; }
  const long n4 = n / 4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    adam1(pp.x, gg.x, mm.x, vv.x, lr, b1, b2, eps, bc1, bc2, wd, decoupled);
    adam1(pp.y, gg.y, mm.y, vv.y, lr, b1, b2, eps, bc1, bc2, wd, decoupled);
    adam1(pp.z, gg.z, mm.z, vv.z, lr, b1, b2, eps, bc1, bc2, wd, decoupled);
    adam1(pp.w, gg.w, mm.w, vv.w, lr, b1, b2, eps, bc1, bc2, wd, decoupled);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (shadow) {
      bf16x4 b = {(bf16)pp.x, (bf16)pp.y, (bf16)pp.z, (bf16)pp.w};
      reinterpret_cast<bf16x4*>(shadow)[i] = b;
    }
  }
  for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam1(pp, g[i], mm, vv, lr, b1, b2, eps, bc1, bc2, wd, decoupled);
    p[i] = pp; m[i] = mm; v[i] = vv;
    if (shadow) shadow[i] = (bf16)pp;
  }
}

// adam_kernel with parameters excluded from weight decay: nodecay holds one byte per 64-element
// block of the flat buffer (arena slices are 64-element aligned, so a block belongs to one
// parameter); a flagged block takes the step with wd = 0. A kernel of its own: adam_kernel, the
// launch of every optimizer without the exclusion, keeps its code. The table is static device
// memory, so a captured step replays it unchanged.
__global__ void adam_nodecay_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                    float* __restrict__ v, bf16* __restrict__ shadow, long n, float lr, float b1,
                                    float b2, float eps, float bc1, float bc2, float wd, int decoupled,
                                    const float* __restrict__ hyper, const uint8_t* __restrict__ nodecay) {
  if (hyper) { lr = hyper[0]; bc1 = hyper[1]; bc2 = hyper[2]; }
  const long n4 = n / 4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float w = nodecay[i >> 4] ? 0.f : wd;
    float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    adam1(pp.x, gg.x, mm.x, vv.x, lr, b1, b2, eps, bc1, bc2, w, decoupled);
    adam1(pp.y, gg.y, mm.y, vv.y, lr, b1, b2, eps, bc1, bc2, w, decoupled);
    adam1(pp.z, gg.z, mm.z, vv.z, lr, b1, b2, eps, bc1, bc2, w, decoupled);
    adam1(pp.w, gg.w, mm.w, vv.w, lr, b1, b2, eps, bc1, bc2, w, decoupled);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (shadow) {
      bf16x4 b = {(bf16)pp.x, (bf16)pp.y, (bf16)pp.z, (bf16)pp.w};
      reinterpret_cast<bf16x4*>(shadow)[i] = b;
    }
  }
  for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam1(pp, g[i], mm, vv, lr, b1, b2, eps, bc1, bc2, nodecay[i >> 6] ? 0.f : wd, decoupled);
    p[i] = pp; m[i] = mm; v[i] = vv;
    if (shadow) shadow[i] = (bf16)pp;
  }
}

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ vel,
                           bf16* __restrict__ shadow, long n, float lr, float mom, const float* __restrict__ hyper) {
  if (hyper) lr = hyper[0];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pp = p[i];
    if (vel) {  // v = mu*v - lr*g ; p += v   (sgd_kernels.cu:27)
      const float vv = mom * vel[i] - lr * g[i];
      vel[i] = vv;
      pp += vv;
    } else {
      pp -= lr * g[i];
    }
    p[i] = pp;
    if (shadow) shadow[i] = (bf16)pp;
  }
}

void adam_step(float* p, const float* g, float* m, float* v, bf16* shadow, long n, float lr, float b1, float b2,
               float eps, float bc1, float bc2, float wd, int decoupled, const float* hyper, hipStream_t s) {
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n / 4 + 1, 256, 4096)), dim3(256), 0, s, p, g, m, v, shadow, n, lr, b1,
                     b2, eps, bc1, bc2, wd, decoupled, hyper);
  DCNN_LAUNCH_CHECK();
}

void adam_step_nodecay(float* p, const float* g, float* m, float* v, bf16* shadow, long n, float lr, float b1, float b2,
                       float eps, float bc1, float bc2, float wd, int decoupled, const float* hyper,
                       const uint8_t* nodecay, hipStream_t s) {
  if (!nodecay) throw std::invalid_argument("adam_step_nodecay: needs the block table ((n + 63) / 64 bytes)");
  hipLaunchKernelGGL(adam_nodecay_kernel, dim3(grid_for(n / 4 + 1, 256, 4096)), dim3(256), 0, s, p, g, m, v, shadow, n,
                     lr, b1, b2, eps, bc1, bc2, wd, decoupled, hyper, nodecay);
  DCNN_LAUNCH_CHECK();
}

// Adam step scalars on the device: t += 1, bc1 = 1 - b1^t, bc2 = 1 - b2^t (hyper = {lr, bc1, bc2, t}).
// Captured in the step graph ahead of adam_kernel, so a replay needs no host upload at all.
__global__ void adam_scalars_kernel(float* hyper, float b1, float b2) {
  if (threadIdx.x == 0) {
    const float t = hyper[3] + 1.f;
    hyper[3] = t;
    hyper[1] = 1.f - powf(b1, t);
    hyper[2] = 1.f - powf(b2, t);
  }
}

void adam_scalars(float* hyper, float b1, float b2, hipStream_t s) {
  hipLaunchKernelGGL(adam_scalars_kernel, dim3(1), dim3(64), 0, s, hyper, b1, b2);
  DCNN_LAUNCH_CHECK();
}

void sgd_step(float* p, const float* g, float* vel, bf16* shadow, long n, float lr, float mom, const float* hyper,
              hipStream_t s) {
  hipLaunchKernelGGL(sgd_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, p, g, vel, shadow, n, lr, mom, hyper);
  DCNN_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------
// Global-norm gradient clipping and weight EMA. grad_sumsq leaves {sumsq, norm, coef, max_norm}
// in device memory (coef = min(1, max_norm / (norm + 1e-6)), torch's clip_grad_norm_); the tail
// kernels are the optimizer step with three optional inputs: the no-decay block table, the clip
// coefficient and the EMA buffer. They are launched only when clip or EMA is on: adam_kernel,
// adam_nodecay_kernel and sgd_kernel above stay the launch of every other optimizer.
// ------------------------------------------------------------------------------------------
// Workgroups of 1024 lanes; float4 loads per lane: 1 while that gives at most 256 workgroups, then
// growing to 60. Few, large workgroups on purpose: the tickets of one launch are taken one after the
// other (about 20 ns each, measured), so their number is kept near one per compute unit while sixteen
// waves per workgroup keep enough loads in flight. A function of n alone, so an eager launch and a
// graph replay add in the same order.
constexpr int kSumsqLanes = 1024;

static int sumsq_per(long n) {
  const long per = (n / 4 + kSumsqLanes * 256L - 1) / (kSumsqLanes * 256L);
  return (int)(per < 1 ? 1 : per > 60 ? 60 : per);
}

int grad_sumsq_blocks(long n) {
  const long span = (long)kSumsqLanes * sumsq_per(n), blocks = (n / 4 + span - 1) / span;
  if (blocks > 0x7fffffffL) throw std::invalid_argument("grad_sumsq: n " + std::to_string(n) + " is too large");
  return (int)(blocks < 1 ? 1 : blocks);
}

__device__ __forceinline__ void clip_block(float* __restrict__ out, float sumsq, float max_norm) {
  const float norm = sqrtf(sumsq), c = max_norm / (norm + 1e-6f);
  out[0] = sumsq;
  out[1] = norm;
  out[2] = c < 1.f || c != c ? c : 1.f;  // fminf(1, c), but a NaN norm propagates (as torch.clamp does)
  out[3] = max_norm;
}

// Each lane keeps four fp32 partials over its `per` float4 loads (61 terms at most in one chain, with
// the scalar tail), then the lane's four, a wave butterfly and the sixteen waves through LDS in a
// fixed tree: one partial per workgroup. The workgroups take a ticket and the last one sums the
// partials in a fixed order, as loss_kernel does: no float atomics, no memset, the ticket word
// resets itself. The trees are 2 + 6 + 4 levels here and 8 in the last workgroup.
__global__ void __launch_bounds__(kSumsqLanes) grad_sumsq_kernel(const float* __restrict__ g, long n, int per,
                                                                 float max_norm, float* part,
                                                                 unsigned* __restrict__ ticket,
                                                                 float* __restrict__ out) {
  __shared__ float sw[16];
  __shared__ float sl[256];
  __shared__ int last;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long n4 = n / 4, base = (long)blockIdx.x * per * kSumsqLanes + threadIdx.x;
  float4 a = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < per; k += 4) {  // four loads in flight; a load past the end adds +0: the bits stay
    float4 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = base + (long)(k + j) * kSumsqLanes;
      x[j] = (k + j < per && i < n4) ? reinterpret_cast<const float4*>(g)[i] : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a.x = __fmaf_rn(x[j].x, x[j].x, a.x);
      a.y = __fmaf_rn(x[j].y, x[j].y, a.y);
      a.z = __fmaf_rn(x[j].z, x[j].z, a.z);
      a.w = __fmaf_rn(x[j].w, x[j].w, a.w);
    }
  }
  if (blockIdx.x == gridDim.x - 1) {  // the scalar tail (n % 4 elements)
    const long i = n4 * 4 + threadIdx.x;
    if (i < n) a.x = __fmaf_rn(g[i], g[i], a.x);
  }
  const float s = wave_sum((a.x + a.y) + (a.z + a.w));
  if (lane == 0) sw[w] = s;
  __syncthreads();
  float blk = 0.f;
  if (threadIdx.x == 0) {  // the sixteen wave sums, pairwise
    float t[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = sw[i];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1)
#pragma unroll
      for (int i = 0; i < o; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    blk = t[0];
  }
  if (gridDim.x == 1) {
    if (threadIdx.x == 0) clip_block(out, blk, max_norm);
    return;
  }
  if (threadIdx.x == 0) {
    part[blockIdx.x] = blk;
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
  // last workgroup: lane t < 256 sums partials t, t + 256, ... in order, then a fixed LDS tree
  if (threadIdx.x < 256) {
    float l = 0.f;
    for (unsigned r = threadIdx.x; r < gridDim.x; r += 256) l += part[r];
    sl[threadIdx.x] = l;
  }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sl[threadIdx.x] += sl[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    clip_block(out, sl[0], max_norm);
    *ticket = 0u;  // ready for the next norm on this stream
  }
}

void grad_sumsq(const float* g, long n, float max_norm, float* part, unsigned* ticket, float* out, hipStream_t s) {
  if (n < 1) throw std::invalid_argument("grad_sumsq: n " + std::to_string(n) + " < 1");
  if (!g || !out || ((uintptr_t)g & 15)) throw std::invalid_argument("grad_sumsq: g (16-byte aligned) and out are required");
  const int blocks = grad_sumsq_blocks(n);
  if (blocks > 1 && (!part || !ticket)) throw std::runtime_error("grad_sumsq: workspace and ticket required");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(kSumsqLanes), 0, s, g, n, sumsq_per(n), max_norm, part, ticket, out);
  DCNN_LAUNCH_CHECK();
}

// The Adam step with its optional inputs, each a wave-uniform null check: nodecay (the block table
// of adam_nodecay_kernel), coef (the clip coefficient grad_sumsq left on the device: the step takes
// g * coef, the gradient buffer is not rewritten) and ema (ema = decay ema + (1 - decay) p_new).
__global__ void adam_tail_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                 float* __restrict__ v, bf16* __restrict__ shadow, long n, float lr, float b1, float b2,
                                 float eps, float bc1, float bc2, float wd, int decoupled,
                                 const float* __restrict__ hyper, const uint8_t* __restrict__ nodecay,
                                 const float* __restrict__ coef, float* __restrict__ ema, float decay) {
  if (hyper) { lr = hyper[0]; bc1 = hyper[1]; bc2 = hyper[2]; }
  const float c = coef ? *coef : 1.f, keep = 1.f - decay;
  const long n4 = n / 4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float w = nodecay && nodecay[i >> 4] ? 0.f : wd;
    float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    if (coef) { gg.x *= c; gg.y *= c; gg.z *= c; gg.w *= c; }
    adam1(pp.x, gg.x, mm.x, vv.x, lr, b1, b2, eps, bc1, bc2, w, decoupled);
    adam1(pp.y, gg.y, mm.y, vv.y, lr, b1, b2, eps, bc1, bc2, w, decoupled);
    adam1(pp.z, gg.z, mm.z, vv.z, lr, b1, b2, eps, bc1, bc2, w, decoupled);
    adam1(pp.w, gg.w, mm.w, vv.w, lr, b1, b2, eps, bc1, bc2, w, decoupled);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (ema) {
      float4 e = reinterpret_cast<float4*>(ema)[i];
      e.x = __fmaf_rn(decay, e.x, keep * pp.x);
      e.y = __fmaf_rn(decay, e.y, keep * pp.y);
      e.z = __fmaf_rn(decay, e.z, keep * pp.z);
      e.w = __fmaf_rn(decay, e.w, keep * pp.w);
      reinterpret_cast<float4*>(ema)[i] = e;
    }
    if (shadow) {
      bf16x4 b = {(bf16)pp.x, (bf16)pp.y, (bf16)pp.z, (bf16)pp.w};
      reinterpret_cast<bf16x4*>(shadow)[i] = b;
    }
  }
  for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pp = p[i], mm = m[i], vv = v[i], gi = g[i];
    if (coef) gi *= c;
    adam1(pp, gi, mm, vv, lr, b1, b2, eps, bc1, bc2, nodecay && nodecay[i >> 6] ? 0.f : wd, decoupled);
    p[i] = pp; m[i] = mm; v[i] = vv;
    if (ema) ema[i] = __fmaf_rn(decay, ema[i], keep * pp);
    if (shadow) shadow[i] = (bf16)pp;
  }
}

// sgd_kernel's arithmetic with the roundings spelled out, so that the vectorised loop cannot contract
// them another way than sgd_kernel's scalar loop is compiled: two products and a difference for the
// velocity, one fma for the plain step. With coef == 1 and no EMA the bits are sgd_kernel's.
__device__ __forceinline__ float sgd1(float& p, float g, float& vel, bool has_vel, float lr, float mom) {
#pragma clang fp contract(off)
  if (has_vel) {
    const float a = mom * vel, b = lr * g;
    const float vv = a - b;
    vel = vv;
    p += vv;
  } else {
    p = __fmaf_rn(-lr, g, p);
  }
  return p;
}

// sgd_kernel with the clip coefficient and the EMA buffer (both optional), 16 bytes per access.
__global__ void sgd_tail_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ vel,
                                bf16* __restrict__ shadow, long n, float lr, float mom, const float* __restrict__ hyper,
                                const float* __restrict__ coef, float* __restrict__ ema, float decay) {
  if (hyper) lr = hyper[0];
  const float c = coef ? *coef : 1.f, keep = 1.f - decay;
  const bool hv = vel != nullptr;
  const long n4 = n / 4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
    float4 vv = {0.f, 0.f, 0.f, 0.f};
    if (hv) vv = reinterpret_cast<float4*>(vel)[i];
    if (coef) { gg.x *= c; gg.y *= c; gg.z *= c; gg.w *= c; }
    sgd1(pp.x, gg.x, vv.x, hv, lr, mom);
    sgd1(pp.y, gg.y, vv.y, hv, lr, mom);
    sgd1(pp.z, gg.z, vv.z, hv, lr, mom);
    sgd1(pp.w, gg.w, vv.w, hv, lr, mom);
    reinterpret_cast<float4*>(p)[i] = pp;
    if (hv) reinterpret_cast<float4*>(vel)[i] = vv;
    if (ema) {
      float4 e = reinterpret_cast<float4*>(ema)[i];
      e.x = __fmaf_rn(decay, e.x, keep * pp.x);
      e.y = __fmaf_rn(decay, e.y, keep * pp.y);
      e.z = __fmaf_rn(decay, e.z, keep * pp.z);
      e.w = __fmaf_rn(decay, e.w, keep * pp.w);
      reinterpret_cast<float4*>(ema)[i] = e;
    }
    if (shadow) {
      bf16x4 b = {(bf16)pp.x, (bf16)pp.y, (bf16)pp.z, (bf16)pp.w};
      reinterpret_cast<bf16x4*>(shadow)[i] = b;
    }
  }
  for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pp = p[i], vv = hv ? vel[i] : 0.f, gi = g[i];
    if (coef) gi *= c;
    sgd1(pp, gi, vv, hv, lr, mom);
    p[i] = pp;
    if (hv) vel[i] = vv;
    if (ema) ema[i] = __fmaf_rn(decay, ema[i], keep * pp);
    if (shadow) shadow[i] = (bf16)pp;
  }
}

// Exchange two flat fp32 buffers and refresh the bf16 shadow from the new a: twice restores every bit.
__global__ void ema_swap_kernel(float* __restrict__ a, float* __restrict__ b, bf16* __restrict__ shadow, long n) {
  const long n4 = n / 4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 x = reinterpret_cast<float4*>(a)[i], y = reinterpret_cast<float4*>(b)[i];
    reinterpret_cast<float4*>(a)[i] = y;
    reinterpret_cast<float4*>(b)[i] = x;
    if (shadow) {
      bf16x4 s = {(bf16)y.x, (bf16)y.y, (bf16)y.z, (bf16)y.w};
      reinterpret_cast<bf16x4*>(shadow)[i] = s;
    }
  }
  for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
    if (shadow) shadow[i] = (bf16)y;
  }
}

static void tail_check(const char* who, const void* p, const void* g, long n, const float* ema, float decay) {
  if (n < 1 || !p || !g) throw std::invalid_argument(std::string(who) + ": p, g and n >= 1 are required");
  if (ema && !(decay > 0.f && decay < 1.f))
    throw std::invalid_argument(std::string(who) + ": ema_decay " + std::to_string(decay) + " is not in (0, 1)");
}

void adam_step_tail(float* p, const float* g, float* m, float* v, bf16* shadow, long n, float lr, float b1, float b2,
                    float eps, float bc1, float bc2, float wd, int decoupled, const float* hyper,
                    const uint8_t* nodecay, const float* coef, float* ema, float decay, hipStream_t s) {
  tail_check("adam_step_tail", p, g, n, ema, decay);
  hipLaunchKernelGGL(adam_tail_kernel, dim3(grid_for(n / 4 + 1, 256, 4096)), dim3(256), 0, s, p, g, m, v, shadow, n, lr,
                     b1, b2, eps, bc1, bc2, wd, decoupled, hyper, nodecay, coef, ema, decay);
  DCNN_LAUNCH_CHECK();
}

void sgd_step_tail(float* p, const float* g, float* vel, bf16* shadow, long n, float lr, float mom, const float* hyper,
                   const float* coef, float* ema, float decay, hipStream_t s) {
  tail_check("sgd_step_tail", p, g, n, ema, decay);
  hipLaunchKernelGGL(sgd_tail_kernel, dim3(grid_for(n / 4 + 1, 256, 4096)), dim3(256), 0, s, p, g, vel, shadow, n, lr,
                     mom, hyper, coef, ema, decay);
  DCNN_LAUNCH_CHECK();
}

void ema_swap(float* a, float* b, bf16* shadow, long n, hipStream_t s) {
  if (n < 1 || !a || !b || a == b) throw std::invalid_argument("ema_swap: two distinct buffers and n >= 1 are required");
  hipLaunchKernelGGL(ema_swap_kernel, dim3(grid_for(n / 4 + 1, 256, 4096)), dim3(256), 0, s, a, b, shadow, n);
  DCNN_LAUNCH_CHECK();
}

}  // namespace dcnn
