// Mixup / CutMix of a device batch with its reverse, in place, plus the dense target: ONE launch.
//
// x is the loader's fp32 [B, C, H, W] batch; sample i is mixed with sample j = B - 1 - i (timm's
// batch mode), one lam and one box per batch (drawn on the host by mix_plan, csrc/native).
//  * Mixup: workgroups over (pair, 2048-float chunk of the row). A lane owns element e of BOTH rows
//    of a pair: it reads both, then writes both, so working in place needs no second buffer. The
//    arithmetic is fma(lam, x_i, (1 - lam) * x_j) with the product rounded on its own - exactly the
//    native CPU backend's, so the two agree bit for bit. 16-byte accesses; a row that is no multiple
//    of 4 floats (or a misaligned base) goes through the same code with 4-byte aligned vectors and a
//    scalar tail.
//  * CutMix: lanes over (c, y, x) INSIDE the box, 4-byte swaps; nothing outside the box is touched,
//    so the traffic is the box's.
//  * A further range of workgroups of the same launch writes the B x K target whole: lam at
//    labels[i], 1 - lam at labels[j], exactly 1 where they agree (and for the middle sample of an odd
//    batch, and in mode 0); a label outside [0, K) contributes nothing.
// No atomics, no LDS, no scratch.
#include "api.h"
#include "common.h"

namespace dcnn {
namespace mix {

constexpr int kChunk = 2048;   // floats of one row per Mixup workgroup (256 lanes x 4 floats x 2)
constexpr int kBoxChunk = 1024;  // box elements of one pair per CutMix workgroup
constexpr int kTgtChunk = 1024;  // target floats per workgroup

struct alignas(4) F4U { float v[4]; };  // 4 floats at a 4-byte aligned address

template <bool ALIGNED>
__device__ __forceinline__ void load4(const float* p, float* f) {
  if (ALIGNED) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    f[0] = t.x; f[1] = t.y; f[2] = t.z; f[3] = t.w;
  } else {
    const F4U t = *reinterpret_cast<const F4U*>(p);
    f[0] = t.v[0]; f[1] = t.v[1]; f[2] = t.v[2]; f[3] = t.v[3];
  }
}
template <bool ALIGNED>
__device__ __forceinline__ void store4(float* p, const float* f) {
  if (ALIGNED) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  } else {
    F4U t;
    t.v[0] = f[0]; t.v[1] = f[1]; t.v[2] = f[2]; t.v[3] = f[3];
    *reinterpret_cast<F4U*>(p) = t;
  }
}

__device__ __forceinline__ float mix1(float l, float o, float a, float b) { return __fmaf_rn(l, a, __fmul_rn(o, b)); }

struct Args {
  float* x;
  const int64_t* labels;
  float* target;
  int B, K, mode;
  int row, HW, W;        // row = C * H * W
  int yl, xl, bh, bw;    // CutMix box origin and extent
  int nbox;              // C * bh * bw
  int per_pair;          // workgroups per pair (Mixup: chunks of the row, CutMix: chunks of the box)
  int mix_blocks;        // pairs * per_pair; the target's workgroups follow
  float lam, oml;        // lam and 1 - lam, both fp32
};

template <bool ALIGNED>
__global__ void __launch_bounds__(256) mix_batch_kernel(const Args p) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= p.mix_blocks) {
    // ---- the dense target
    const long total = (long)p.B * p.K;
    const long base = (long)(blockIdx.x - p.mix_blocks) * kTgtChunk;
    if (ALIGNED && (p.K & 3) == 0) {
      const long e = base + tid * 4l;
      if (e < total) {
        const int i = (int)(e / p.K), k0 = (int)(e % p.K);
        const int64_t a = p.labels[i], b = p.labels[p.B - 1 - i];
        const bool one = a == b || p.mode == 0 || p.B - 1 - i == i;
        float f[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int64_t k = k0 + v;
          f[v] = one ? (k == a ? 1.0f : 0.f) : (k == a ? p.lam : (k == b ? p.oml : 0.f));
        }
        store4<true>(p.target + e, f);
      }
    } else {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const long e = base + it * 256 + tid;
        if (e < total) {
          const int i = (int)(e / p.K);
          const int64_t k = e % p.K;
          const int64_t a = p.labels[i], b = p.labels[p.B - 1 - i];
          const bool one = a == b || p.mode == 0 || p.B - 1 - i == i;
          p.target[e] = one ? (k == a ? 1.0f : 0.f) : (k == a ? p.lam : (k == b ? p.oml : 0.f));
        }
      }
    }
    return;
  }
  const int pair = blockIdx.x / p.per_pair, chunk = blockIdx.x % p.per_pair;
  float* xi = p.x + (long)pair * p.row;
  float* xj = p.x + (long)(p.B - 1 - pair) * p.row;
  if (p.mode == 1) {
    // ---- Mixup: both loads of both iterations first, then the stores
    const int e0 = chunk * kChunk + tid * 4, e1 = e0 + 1024;
    float a0[4], b0[4], a1[4], b1[4];
    const bool v0 = e0 + 4 <= p.row, v1 = e1 + 4 <= p.row;
    if (v0) { load4<ALIGNED>(xi + e0, a0); load4<ALIGNED>(xj + e0, b0); }
    if (v1) { load4<ALIGNED>(xi + e1, a1); load4<ALIGNED>(xj + e1, b1); }
    if (v0) {
      float r[4], q[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) { r[v] = mix1(p.lam, p.oml, a0[v], b0[v]); q[v] = mix1(p.lam, p.oml, b0[v], a0[v]); }
      store4<ALIGNED>(xi + e0, r);
      store4<ALIGNED>(xj + e0, q);
    } else {
      for (int e = e0; e < p.row && e < e0 + 4; ++e) {  // the scalar tail of the row
        const float a = xi[e], b = xj[e];
        xi[e] = mix1(p.lam, p.oml, a, b);
        xj[e] = mix1(p.lam, p.oml, b, a);
      }
    }
    if (v1) {
      float r[4], q[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) { r[v] = mix1(p.lam, p.oml, a1[v], b1[v]); q[v] = mix1(p.lam, p.oml, b1[v], a1[v]); }
      store4<ALIGNED>(xi + e1, r);
      store4<ALIGNED>(xj + e1, q);
    } else {
      for (int e = e1; e < p.row && e < e1 + 4; ++e) {
        const float a = xi[e], b = xj[e];
        xi[e] = mix1(p.lam, p.oml, a, b);
        xj[e] = mix1(p.lam, p.oml, b, a);
      }
    }
  } else {
    // ---- CutMix: swap the box, 4 elements per lane
    const int plane = p.bh * p.bw;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int q = chunk * kBoxChunk + it * 256 + tid;
      if (q < p.nbox) {
        const int c = q / plane, r = q % plane;
        const int o = c * p.HW + (p.yl + r / p.bw) * p.W + p.xl + r % p.bw;
        const float a = xi[o], b = xj[o];
        xi[o] = b;
        xj[o] = a;
      }
    }
  }
}

}  // namespace mix

void mix_batch(float* x, const int64_t* labels, float* target, int B, int C, int H, int W, int mode, float lam, int yl,
               int yh, int xl, int xh, int K, hipStream_t s) {
  auto bad = [](const std::string& m) { throw std::invalid_argument("mix_batch: " + m); };
  if (B < 1 || C < 1 || H < 1 || W < 1)
    bad("empty batch " + std::to_string(B) + "x" + std::to_string(C) + "x" + std::to_string(H) + "x" + std::to_string(W));
  if ((double)B * C * H * W > 2147483647.0) bad(std::to_string((double)B * C * H * W) + " elements exceed 2^31 - 1");
  if (K < 1) bad("num_classes " + std::to_string(K) + " < 1");
  if ((double)B * K > 2147483647.0) bad(std::to_string((double)B * K) + " target elements exceed 2^31 - 1");
  if (mode < 0 || mode > 2) bad("mode " + std::to_string(mode) + " is not 0, 1 or 2");
  if (!(lam >= 0.f && lam <= 1.f)) bad("lam " + std::to_string(lam) + " is not in [0, 1]");
  if (mode == 2 && !(0 <= yl && yl <= yh && yh <= H && 0 <= xl && xl <= xh && xh <= W))
    bad("box [" + std::to_string(yl) + ", " + std::to_string(yh) + ") x [" + std::to_string(xl) + ", " +
        std::to_string(xh) + ") is outside the " + std::to_string(H) + "x" + std::to_string(W) + " image");
  if (!labels || !target || (mode != 0 && !x)) bad("null pointer");
  if (((uintptr_t)x & 3) || ((uintptr_t)target & 3)) bad("x and target must be 4-byte aligned");
  mix::Args a{};
  a.x = x; a.labels = labels; a.target = target;
  a.B = B; a.K = K; a.mode = mode;
  a.row = C * H * W; a.HW = H * W; a.W = W;
  a.lam = mode == 0 ? 1.0f : lam;
  a.oml = 1.0f - a.lam;
  const long pairs = B / 2;
  if (mode == 1) {
    a.per_pair = (a.row + mix::kChunk - 1) / mix::kChunk;
  } else if (mode == 2) {
    a.yl = yl; a.xl = xl; a.bh = yh - yl; a.bw = xh - xl;
    a.nbox = C * a.bh * a.bw;
    a.per_pair = (a.nbox + mix::kBoxChunk - 1) / mix::kBoxChunk;
  }
  const long mb = pairs * a.per_pair;
  const long tb = ((long)B * K + mix::kTgtChunk - 1) / mix::kTgtChunk;
  if (mb + tb > 2147483647l) bad("too many workgroups");
  a.mix_blocks = (int)mb;
  const bool aligned = (a.row & 3) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)target & 15) == 0;
  if (aligned)
    mix::mix_batch_kernel<true><<<dim3((unsigned)(mb + tb)), dim3(256), 0, s>>>(a);
  else
    mix::mix_batch_kernel<false><<<dim3((unsigned)(mb + tb)), dim3(256), 0, s>>>(a);
  DCNN_LAUNCH_CHECK();
}

}  // namespace dcnn
