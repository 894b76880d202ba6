// The classifier head in two launches (bf16 NHWC, fp32 accumulation on mfma_f32_16x16x32_bf16):
//
//   head_fwd   global average pool + FC + bias   x[N][HW][In] -> pooled[N][In], logits[N][Out]
//   head_bwd   FC data gradient + pool backward  dlogits, W   -> dx[N][HW][In]           (data blocks)
//              FC weight and bias gradients      dlogits, pooled -> slab / bias_slab       (weight blocks)
//
// The separate path is global_avgpool_fwd + gemm_nt, and conv_weight_transpose + gemm_nt +
// gemm_tn + global_avgpool_bwd: six kernels whose whole duration is launch, prologue and drain
// latency around 3 x 52 MFLOP. The fused kernels round to bf16 where those kernels do: the pooled
// value (sum over the pixels in order, / HW), the logits (accumulator + fp32 bias), the pooled
// gradient, and the pooled gradient x 1/HW. W[Out][In] is read as stored: the data gradient
// contracts over Out through an LDS transpose of its W slice, so no [In][Out] copy is built.
// Every sum has a fixed order; there are no float atomics.
//
// MFMA operand maps (16x16x32 bf16): lane l holds A[row l & 15][k = 8 (l >> 4) + j] and
// B[k = 8 (l >> 4) + j][col l & 15], j = 0..7; result reg j is D[row 4 (l >> 4) + j][col l & 15].
#include <algorithm>

#include "api.h"
#include "common.h"

namespace dcnn {
namespace {

constexpr int kImgs = 16;        // images per data block and at most per forward workgroup (one MFMA row tile)
constexpr int kFwdThreads = 512;
constexpr int kFwdCls = 128;     // classes per forward workgroup: 16 per wave
constexpr int kBwdThreads = 256;
constexpr int kMaxIn = 2048;     // forward LDS tile [16][In] bf16 = 64 KB
constexpr int kKC = 256;         // data blocks: classes staged per pass
constexpr int kLdD = kKC + 8;    // their LDS row stride (elements): 16-byte reads 4 banks apart
constexpr int kLdW = 64 + 8;     // weight blocks: LDS row stride of the 64-image chunk

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 ld8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

// pooled tile in LDS: row r's 16-byte chunk c sits at chunk c ^ (r & 7), so the 16 rows an MFMA
// operand read touches spread over the banks without padding the 64 KB tile
__device__ __forceinline__ int swz(int r, int c) { return c ^ (r & 7); }

// data-block W slice, transposed: element (input channel i of 64, class k) — every group of 8
// rows shifted by one 16-byte chunk, so the 8 x 2-byte transposing writes of a lane group and
// the 16-byte operand reads both spread over the banks
__device__ __forceinline__ int wt_at(int i, int k) { return i * kLdD + (i >> 3) * 8 + k; }

constexpr int kSmemData = (kImgs * kLdD + 64 * kLdD + 64 + kImgs * 64) * 2;
constexpr int kSmemWeight = 2 * 64 * kLdW * 2;
constexpr int kSmemBwd = kSmemData > kSmemWeight ? kSmemData : kSmemWeight;

}  // namespace

__global__ __launch_bounds__(kFwdThreads) void head_fwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                               const float* __restrict__ bias,
                                                               bf16* __restrict__ pooled, bf16* __restrict__ logits,
                                                               int N, int HW, int In, int Out, int ipb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char head_smem[];
  bf16* tile = reinterpret_cast<bf16*>(head_smem);  // [16][In]
  const int n0 = blockIdx.x * ipb, nend = min(N, n0 + ipb);  // (rows past ipb: zero operands)
  const int chunks = In >> 3;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int c0 = blockIdx.y * kFwdCls + wave * 16;  // this wave's 16 classes
  const bool wave_on = c0 < Out;
  const int cls = c0 + r;
  const bool cok = cls < Out;
  // (a class column past Out computes on row 0 of w and is never stored)
  const bf16* wr = w + (long)(cok ? cls : 0) * In + g * 8;
  const int k64 = In >> 6;  // (In % 64 == 0)
  // this lane's W operands of 512 input channels, in registers; the first 512 are requested
  // before the pool so that their latency hides behind the pool's
  bf16x8 b[16];
  auto load_w = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int kq = min(k0 + u, k64 - 1);  // (past In: loaded again, not used)
      b[2 * u] = ld8(wr + kq * 64);
      b[2 * u + 1] = ld8(wr + kq * 64 + 32);
    }
  };
  if (wave_on) load_w(0);

  // average pool: one (image, 8 channels) item per thread and step, pixels summed in order
  for (int it = threadIdx.x; it < kImgs * chunks; it += kFwdThreads) {
    const int pr = it / chunks, c = it - pr * chunks;
    const int n = n0 + pr;
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    if (n < nend) {
      const uint4* px = reinterpret_cast<const uint4*>(x + (long)n * HW * In) + c;
      for (int p0 = 0; p0 < HW; p0 += 8) {
        uint4 u[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) u[q] = p0 + q < HW ? px[(long)(p0 + q) * chunks] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float f[8];
          unpack8(u[q], f);
#pragma unroll
          for (int e = 0; e < 8; ++e) s[e] += f[e];
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = s[e] / (float)HW;
    }
    const uint4 o = pack8(s);
    *reinterpret_cast<uint4*>(tile + pr * In + swz(pr, c) * 8) = o;
    if (blockIdx.y == 0 && n < nend) *reinterpret_cast<uint4*>(pooled + (long)n * In + c * 8) = o;
  }
  __syncthreads();
  if (!wave_on) return;  // (whole wave, after the only barrier)

  const bf16* ar = tile + r * In;
  // one accumulator, 32 input channels per MFMA in ascending order: gemm_nt's chain, so the
  // logits are the bits the separate FC forward stores
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < k64; k0 += 8) {
    if (k0 > 0) load_w(k0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (k0 + u < k64) {
        acc = mfma16(ld8(ar + swz(r, (k0 + u) * 8 + g) * 8), b[2 * u], acc);
        acc = mfma16(ld8(ar + swz(r, (k0 + u) * 8 + 4 + g) * 8), b[2 * u + 1], acc);
      }
    }
  }
  if (!cok) return;
  const float bv = bias ? bias[cls] : 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + g * 4 + j;
    if (n < nend) logits[(long)n * Out + cls] = (bf16)(acc[j] + bv);
  }
}

__global__ __launch_bounds__(kBwdThreads) void head_bwd_kernel(const bf16* __restrict__ dl, const bf16* __restrict__ w,
                                                               const bf16* __restrict__ pooled, bf16* __restrict__ dx,
                                                               float* __restrict__ slab, float* __restrict__ bslab,
                                                               int N, int HW, int In, int Out, int n_data, int per,
                                                               int brows) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kSmemBwd];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, g = lane >> 4;
  const int tiles_i = In >> 6;
  const bf16 bz = (bf16)0.f;

  if ((int)blockIdx.x < n_data) {
    // ---- data block: 16 images x 64 input channels of dx --------------------------------
    bf16* sdl = reinterpret_cast<bf16*>(smem);  // [16][kLdD] dlogits rows, zero-padded
    bf16* swt = sdl + kImgs * kLdD;             // [64][kLdD] (+ group shifts) W slice transposed
    bf16* sout = swt + 64 * kLdD + 64;          // [16][64] the pooled gradient x 1/HW
    const int ib = blockIdx.x / tiles_i, cb = blockIdx.x - ib * tiles_i;
    const int n0 = ib * kImgs, i0 = cb * 64;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int o0 = 0; o0 < Out; o0 += kKC) {
      const int kc = min(kKC, Out - o0);
      const int kp = (kc + 31) & ~31;  // classes past Out: zero operands
      if (o0 > 0) __syncthreads();
      // every global load of the pass is requested before the first LDS write waits for one:
      // 8 x 16 bytes of the W slice (class k = tid / 8 + 32 it, 8 channels) and 16 dlogits
      // elements (image tid / 16, class tid % 16 + 16 it) per thread
      uint4 wv[kKC / 32];
      bf16 dv[kKC / 16];
      const int c8 = tid & 7, dr = tid >> 4;
#pragma unroll
      for (int it = 0; it < kKC / 32; ++it) {
        const int k = (tid >> 3) + 32 * it;
        wv[it] = k < kc ? *reinterpret_cast<const uint4*>(w + (long)(o0 + k) * In + i0 + c8 * 8) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int it = 0; it < kKC / 16; ++it) {
        const int k = (tid & 15) + 16 * it;
        dv[it] = (n0 + dr < N && k < kc) ? dl[(long)(n0 + dr) * Out + o0 + k] : bz;
      }
#pragma unroll
      for (int it = 0; it < kKC / 32; ++it) {
        const int k = (tid >> 3) + 32 * it;
        const bf16* v = reinterpret_cast<const bf16*>(&wv[it]);
        if (k < kp) {
#pragma unroll
          for (int j = 0; j < 8; ++j) swt[wt_at(c8 * 8 + j, k)] = v[j];
        }
      }
#pragma unroll
      for (int it = 0; it < kKC / 16; ++it) {
        const int k = (tid & 15) + 16 * it;
        if (k < kp) sdl[dr * kLdD + k] = dv[it];
      }
      __syncthreads();
      for (int kb = 0; kb < kp / 32; ++kb)
        acc = mfma16(ld8(sdl + r * kLdD + kb * 32 + g * 8), ld8(swt + wt_at(wave * 16 + r, kb * 32 + g * 8)), acc);
    }
    const float inv = 1.f / (float)HW;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16 dp = (bf16)(acc[j] + 0.f);  // the pooled gradient as the FC data gradient stores it (no bias: + 0)
      sout[(g * 4 + j) * 64 + wave * 16 + r] = (bf16)((float)dp * inv);
    }
    __syncthreads();
    const int total = kImgs * HW * 8;
    for (int e = tid; e < total; e += kBwdThreads) {
      const int c8 = e & 7, q = e >> 3;
      const int rr = q / HW, p = q - rr * HW;
      const int n = n0 + rr;
      if (n < N)
        *reinterpret_cast<uint4*>(dx + ((long)n * HW + p) * In + i0 + c8 * 8) =
            *reinterpret_cast<const uint4*>(sout + rr * 64 + c8 * 8);
    }
    return;
  }

  // ---- weight block: 64 classes x 64 input channels of one batch split ----------------------
  bf16* sa = reinterpret_cast<bf16*>(smem);  // [64 classes][kLdW] dlogits chunk, transposed
  bf16* sb = sa + 64 * kLdW;                 // [64 inputs][kLdW] pooled chunk, transposed
  const int wb = blockIdx.x - n_data;
  const int tiles_o = (Out + 63) >> 6;
  const int split = wb / (tiles_o * tiles_i), t = wb - split * tiles_o * tiles_i;
  const int ob = t / tiles_i, cb = t - ob * tiles_i;
  const int o0 = ob * 64, i0 = cb * 64;
  const int nbeg = split * per, nend = min(N, nbeg + per);
  f32x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bpart[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = nbeg; c0 < nend; c0 += 64) {
    if (c0 > nbeg) __syncthreads();
    // all of the chunk's global loads first (2 x 16 bytes of pooled, 16 dlogits elements per
    // thread: class tid % 64, image tid / 64 + 4 it), then the transposing LDS writes
    uint4 pv[2];
    bf16 dv[16];
    const int c8 = tid & 7, o = tid & 63;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int nn = (tid >> 3) + 32 * it;
      pv[it] = c0 + nn < nend ? *reinterpret_cast<const uint4*>(pooled + (long)(c0 + nn) * In + i0 + c8 * 8)
                              : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int nn = (tid >> 6) + 4 * it;
      dv[it] = (c0 + nn < nend && o0 + o < Out) ? dl[(long)(c0 + nn) * Out + o0 + o] : bz;
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int nn = (tid >> 3) + 32 * it;
      const bf16* v = reinterpret_cast<const bf16*>(&pv[it]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sb[(c8 * 8 + j) * kLdW + nn] = v[j];
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) sa[o * kLdW + (tid >> 6) + 4 * it] = dv[it];
    __syncthreads();
    // (gemm_tn's chain: one accumulator, two MFMAs of 32 images per 64-image chunk, rows past the
    // split zero)
    for (int kb = 0; kb < 2; ++kb) {
      const bf16x8 a = ld8(sa + (wave * 16 + r) * kLdW + kb * 32 + g * 8);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = mfma16(a, ld8(sb + (q * 16 + r) * kLdW + kb * 32 + g * 8), acc[q]);
    }
    // bias gradient: gemm_tn's column sums — brows interleaved partials per class (chunk row r
    // goes to partial r % brows, rows and chunks in ascending order), added in order at the end
    if (bslab != nullptr && cb == 0 && tid < 64) {
      if (brows == 2) {
        for (int nn = 0; nn < 64; ++nn) bpart[nn & 1] += (float)sa[tid * kLdW + nn];
      } else {
        for (int nn = 0; nn < 64; ++nn) bpart[nn & 3] += (float)sa[tid * kLdW + nn];
      }
    }
  }
  float* out = slab + (long)split * Out * In;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int o = o0 + wave * 16 + g * 4 + j;
    if (o < Out) {
#pragma unroll
      for (int q = 0; q < 4; ++q) out[(long)o * In + i0 + q * 16 + r] = acc[q][j];
    }
  }
  if (bslab != nullptr && cb == 0 && tid < 64 && o0 + tid < Out) {
    float bsum = 0.f;
    for (int k = 0; k < brows; ++k) bsum += bpart[k];
    bslab[(long)split * Out + o0 + tid] = bsum;
  }
}

namespace {

void check_head(PoolGeom g, int Out) {
  if (!head_supported(g, Out))
    throw std::invalid_argument("head: needs a whole-map average pool without padding, In % 64 == 0, In <= 2048, "
                                "N >= 1, Out >= 1");
}

// The weight blocks split the batch exactly as gemm_tn splits it for the same FC (gemm_tn_splits,
// 64-image chunks), run the same MFMA chain per split and sum the bias partials in its order, so
// the slabs — and after the unchanged reduce the gradients — are the separate path's bits.
int head_per(int N, int In, int Out) { return gemm_tn_k_per_split(N, gemm_tn_splits(Out, In, N)); }

}  // namespace

bool head_supported(PoolGeom g, int Out) {
  return g.N >= 1 && Out >= 1 && g.H >= 1 && g.W >= 1 && g.OH == 1 && g.OW == 1 && g.ph == g.H && g.pw == g.W &&
         g.padh == 0 && g.padw == 0 && g.C >= 64 && g.C % 64 == 0 && g.C <= kMaxIn &&
         (long)g.N * g.H * g.W * g.C < (1l << 31) && (long)Out * g.C < (1l << 31) && (long)g.N * Out < (1l << 31);
}

void head_fwd(const bf16* x, const bf16* w, const float* bias, bf16* pooled, bf16* logits, PoolGeom g, int Out,
              hipStream_t s) {
  check_head(g, Out);
  // images per workgroup: the pool is the kernel's memory traffic and its latency is per
  // workgroup, so small batches spread it over more workgroups (MFMA rows past ipb are zero)
  int ipb = kImgs;
  while (ipb > 2 && (g.N + ipb - 1) / ipb < 32) ipb /= 2;
  const dim3 grid((g.N + ipb - 1) / ipb, (Out + kFwdCls - 1) / kFwdCls);
  hipLaunchKernelGGL(head_fwd_kernel, grid, dim3(kFwdThreads), (size_t)kImgs * g.C * 2, s, x, w, bias, pooled, logits,
                     g.N, g.H * g.W, g.C, Out, ipb);
  DCNN_LAUNCH_CHECK();
}

int head_bwd_splits(int N, int In, int Out) { return gemm_tn_splits(Out, In, N); }

void head_bwd(const bf16* dlogits, const bf16* w, const bf16* pooled, bf16* dx, float* slab, float* bias_slab,
              PoolGeom g, int Out, hipStream_t s) {
  check_head(g, Out);
  const int tiles_i = g.C / 64;
  const int n_data = dx != nullptr ? (g.N + kImgs - 1) / kImgs * tiles_i : 0;
  const int n_weight = head_bwd_splits(g.N, g.C, Out) * ((Out + 63) / 64) * tiles_i;
  hipLaunchKernelGGL(head_bwd_kernel, dim3(n_data + n_weight), dim3(kBwdThreads), 0, s, dlogits, w, pooled, dx, slab,
                     bias_slab, g.N, g.H * g.W, g.C, Out, n_data, head_per(g.N, g.C, Out),
                     gemm_tn_bias_rows(Out));
  DCNN_LAUNCH_CHECK();
}

}  // namespace dcnn
