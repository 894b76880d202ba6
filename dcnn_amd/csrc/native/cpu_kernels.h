// Native CPU compute backend (host side of the framework; the GPU side is csrc/kernels/*.hip).
//
// Reference: src/math/cpu/sgemm.cpp / dgemm.cpp (blocked GEMM), src/ops/cpu/skernels.cpp /
// dkernels.cpp (elementwise + reductions), include/tensor/cpu/tensor_ops.hpp (im2col/col2im/pad),
// src/nn/layers_impl/cpu/*_ops.cpp (conv, batchnorm, pooling). Every routine is templated on
// float/double, runs on the native ThreadPool, and is deterministic (fixed chunking, fixed
// reduction order). Layouts are NCHW contiguous, as in the reference's CPU path.
#pragma once
#include <cstdint>

namespace dcnn_native {
namespace cpu {

// C[M,N] = alpha * op(A)[M,K] @ op(B)[K,N] + beta * C   (row-major; ta/tb transpose A/B)
void gemm(bool ta, bool tb, long M, long N, long K, float alpha, const float* A, long lda, const float* B, long ldb,
          float beta, float* C, long ldc);
void gemm(bool ta, bool tb, long M, long N, long K, double alpha, const double* A, long lda, const double* B, long ldb,
          double beta, double* C, long ldc);
bool gemm_uses_avx2();
bool gemm_uses_avx512();

template <typename T> void elementwise(int mode, int op, const T* a, const T* b, T* c, long n, double s0, double s1);
template <typename T> double reduce(int op, const T* a, const T* b, long n);
template <typename T> void fill_random(T* out, long n, uint64_t seed, double a, double b, int normal);
template <typename T> void transpose2d(const T* in, T* out, long batch, long rows, long cols);
template <typename T> void swap01(const T* in, T* out, long A, long B, long HW);
template <typename T> void pad2d(const T* x, T* y, long NC, int H, int W, int ph, int pw, double value);
template <typename T> void crop2d(const T* x, T* y, long NC, int H, int W, int top, int left, int OH, int OW);
template <typename T>
void im2col(const T* x, T* col, int N, int C, int H, int W, int KH, int KW, int SH, int SW, int PH, int PW);
template <typename T>
void col2im(const T* col, T* x, int N, int C, int H, int W, int KH, int KW, int SH, int SW, int PH, int PW);
template <typename T>
void conv2d_fwd(const T* x, const T* w, const T* bias, T* y, int N, int C, int H, int W, int Co, int KH, int KW, int SH,
                int SW, int PH, int PW);
template <typename T>
void conv2d_bwd(const T* x, const T* w, const T* dy, T* dx, T* dw, T* db, int N, int C, int H, int W, int Co, int KH,
                int KW, int SH, int SW, int PH, int PW);
// depthwise (groups = C, multiplier 1): w [C][KH][KW]; bwd: dx overwritten (may be null), dw / db +=
template <typename T>
void depthwise_conv2d_fwd(const T* x, const T* w, const T* bias, T* y, int N, int C, int H, int W, int KH, int KW,
                          int SH, int SW, int PH, int PW);
template <typename T>
void depthwise_conv2d_bwd(const T* x, const T* w, const T* dy, T* dx, T* dw, T* db, int N, int C, int H, int W, int KH,
                          int KW, int SH, int SW, int PH, int PW);
// grouped (1 < G < C): w [Co][C / G][KH][KW]; bwd: dx overwritten (may be null), dw / db +=
template <typename T>
void grouped_conv2d_fwd(const T* x, const T* w, const T* bias, T* y, int N, int C, int H, int W, int Co, int G, int KH,
                        int KW, int SH, int SW, int PH, int PW);
template <typename T>
void grouped_conv2d_bwd(const T* x, const T* w, const T* dy, T* dx, T* dw, T* db, int N, int C, int H, int W, int Co,
                        int G, int KH, int KW, int SH, int SW, int PH, int PW);
template <typename T> void dense_fwd(const T* x, const T* w, const T* bias, T* y, long N, long In, long Out);
template <typename T>
void dense_bwd(const T* x, const T* w, const T* dy, T* dx, T* dw, T* db, long N, long In, long Out);
template <typename T>
void batchnorm_fwd(const T* x, T* y, long N, long C, long HW, const T* gamma, const T* beta, double eps, int training,
                   T* running_mean, T* running_var, double momentum, T* save_mean, T* save_istd, int relu,
                   const T* residual);
template <typename T>
void batchnorm_bwd(const T* x, const T* dy, const T* yout, const T* mean, const T* istd, const T* gamma, T* dx,
                   T* dgamma, T* dbeta, T* masked_out, long N, long C, long HW, int training);
template <typename T>
void groupnorm_fwd(const T* x, T* y, long N, long C, long HW, long G, const T* gamma, const T* beta, double eps,
                   T* save_mean, T* save_istd);
template <typename T>
void groupnorm_bwd(const T* x, const T* dy, const T* mean, const T* istd, const T* gamma, T* dx, T* dgamma, T* dbeta,
                   long N, long C, long HW, long G);
// channel LayerNorm: every (n, position) over its C channels; statistics [N][HW]; dgamma / dbeta +=
template <typename T>
void layernorm_fwd(const T* x, T* y, long N, long C, long HW, const T* gamma, const T* beta, double eps, T* save_mean,
                   T* save_rstd);
template <typename T>
void layernorm_bwd(const T* x, const T* dy, const T* mean, const T* rstd, const T* gamma, T* dx, T* dgamma, T* dbeta,
                   long N, long C, long HW);
// y = gamma[c] x (+ residual); dx = gamma[c] dy (may be null), dgamma += (may be null)
template <typename T>
void layer_scale_fwd(const T* x, const T* gamma, const T* residual, T* y, long N, long C, long HW);
template <typename T>
void layer_scale_bwd(const T* x, const T* dy, const T* gamma, T* dx, T* dgamma, long N, long C, long HW);
template <typename T>
void maxpool_fwd(const T* x, T* y, int32_t* idx, long NC, int H, int W, int KH, int KW, int SH, int SW, int PH, int PW);
template <typename T> void maxpool_bwd(const T* dy, const int32_t* idx, T* dx, long NC, int H, int W, int OH, int OW);
template <typename T>
void avgpool_fwd(const T* x, T* y, long NC, int H, int W, int KH, int KW, int SH, int SW, int PH, int PW);
template <typename T>
void avgpool_bwd(const T* dy, T* dx, long NC, int H, int W, int KH, int KW, int SH, int SW, int PH, int PW);
template <typename T> void act_fwd(int type, const T* x, T* y, long n, double alpha);
template <typename T> void act_bwd(int type, const T* x, const T* dy, T* dx, long n, double alpha);
template <typename T> void softmax_channels(const T* x, T* y, long N, long C, long HW);
template <typename T> void softmax_channels_bwd(const T* y, const T* dy, T* dx, long N, long C, long HW);
template <typename T>
double loss_fused(int kind, const T* pred, const T* target, const int64_t* labels, T* grad, long N, long C,
                  double param, long* correct);
template <typename T> void sgd_step(T* p, const T* g, T* vel, long n, double lr, double momentum);
template <typename T>
void adam_step(T* p, const T* g, T* m, T* v, long n, double lr, double b1, double b2, double eps, double bc1,
               double bc2, double wd, int decoupled);
// adam_step, with wd = 0 for every 64-element block whose byte in nodecay [(n + 63) / 64] is set
template <typename T>
void adam_step_nodecay(T* p, const T* g, T* m, T* v, long n, double lr, double b1, double b2, double eps, double bc1,
                       double bc2, double wd, int decoupled, const uint8_t* nodecay);
// Global-norm clipping and weight EMA. grad_sumsq: sum of g^2 in a fixed order (double partials).
// The tail steps are adam_step / sgd_step with optional inputs, null = off: nodecay (as above), coef
// (the step takes g * coef, g is left as it is), ema (ema = decay ema + (1 - decay) p_new).
template <typename T> double grad_sumsq(const T* g, long n);
template <typename T>
void adam_step_tail(T* p, const T* g, T* m, T* v, long n, double lr, double b1, double b2, double eps, double bc1,
                    double bc2, double wd, int decoupled, const uint8_t* nodecay, const double* coef, T* ema,
                    double decay);
template <typename T>
void sgd_step_tail(T* p, const T* g, T* vel, long n, double lr, double momentum, const double* coef, T* ema,
                   double decay);
template <typename T> void ema_swap(T* a, T* b, long n);
// Layer-wise optimizers over the flat buffer, driven by the GPU's segment / chunk tables
// (csrc/kernels/optim_segments.h) as flat int32 rows: chunks [nchunks][3] = {first 64-element block,
// blocks, segment}, segs [nsegs][4] = {first chunk, chunks, adapt, decay}. Norms are double partials per
// chunk in element order, added per segment in chunk order. out [3 nsegs]: trust, then {sum p^2, sum
// u^2} per segment. LAMB: r = (m / bc1) / (sqrt(v / bc2) + eps) + wd_i p, p -= lr trust_i r, trust_i =
// ||p_i|| / ||r_i||. LARS: trust_i = tc ||p_i|| / (coef ||g_i|| + wd_i ||p_i|| + eps), v = mom v - lr
// trust_i (g + wd_i p), p += v. trust_i = 1 where the segment does not adapt or a norm is zero; a
// non-finite norm propagates. coef / ema as in the tail steps.
template <typename T>
void lamb_step(T* p, const T* g, T* m, T* v, long n, double lr, double b1, double b2, double eps, double bc1,
               double bc2, double wd, const double* coef, T* ema, double decay, const int* chunks, int nchunks,
               const int* segs, int nsegs, double* out);
template <typename T>
void lars_step(T* p, const T* g, T* vel, long n, double lr, double momentum, double wd, double tc, double eps,
               const double* coef, T* ema, double decay, const int* chunks, int nchunks, const int* segs, int nsegs,
               double* out);
// stochastic depth: mask[n] = 0 or 1 / (1 - p), the GPU's mask (csrc/kernels/droppath.hip) bit for
// bit; y[n][:] = mask[n] x[n][:] over samples of `row` contiguous elements
void drop_path_mask(float* mask, long N, double p, uint64_t seed, uint64_t draw);
template <typename T> void drop_path_scale(const T* x, const float* mask, T* y, long N, long row);

// Mixup / CutMix. mix_plan: the per-batch draw, a pure function of (seed, step) - the only place
// either front end draws. mode 0 none, 1 Mixup, 2 CutMix with the box [yl, yh) x [xl, xh).
// mix_batch: x [B, C, H, W] mixed in place with the reversed batch, target [B, K] fp32 written
// whole; the GPU kernel's rounding (csrc/kernels/mix.hip), bit for bit. mix_check: the argument
// checks both backends share (throws std::invalid_argument naming the value).
struct MixPlan {
  int mode;
  double lam;
  int yl, yh, xl, xh;
};
MixPlan mix_plan(uint64_t seed, uint64_t step, int H, int W, double mixup_alpha, double cutmix_alpha, double prob,
                 double switch_prob);
void mix_check(long B, long C, long H, long W, long K, int mode, double lam, int yl, int yh, int xl, int xh);
template <typename T>
void mix_batch(T* x, const int64_t* labels, float* target, long B, long C, long H, long W, int mode, double lam,
               int yl, int yh, int xl, int xh, long K);

}  // namespace cpu
}  // namespace dcnn_native
