// C ABI over the C++ host API's GPU convolution entry points (dcnn/ops.hpp gpu_ops), for tests that
// drive the C++ engine's own plumbing from Python (ctypes on libdcnn.so, device pointers of torch
// tensors): tests/test_gpu_cpp_geometry.py replays every conv call a production C++ training step
// records (DCNN_RECORD_OPS) through these functions and compares with fp32 PyTorch.
//
// Every call runs on the calling thread's flow and synchronises the device before it returns (the
// caller synchronises its own stream before the call). Returns 0, or -1 with dcnn_c_last_error().
// shape[13] = ConvShape {N, C, H, W, Co, KH, KW, SH, SW, PH, PW, OH, OW}.
// Reference parity: unit_tests/conv2d_layer_test.cpp:660-990 drives the reference's conv layer the
// same way (per-shape calls against a loop reference).
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>

#include "../kernels/optim_segments.h"
#include "dcnn/ops.hpp"
#include "dcnn/tensor.hpp"

using namespace dcnn;

namespace {
thread_local std::string t_err;

ConvShape shape_of(const int* v) {
  return ConvShape{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12]};
}

template <typename F>
int guarded(F&& f) {
  try {
    f();
    gpu::synchronize();
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  } catch (...) {
    t_err = "unknown error";
  }
  return -1;
}
}  // namespace

extern "C" {

const char* dcnn_c_last_error() { return t_err.c_str(); }

void dcnn_c_set_fault(int f) { gpu_ops::set_fault(f); }

int dcnn_c_copy(void* dst, const void* src, size_t nbytes) {
  return guarded([&] { gpu::copy(dst, src, nbytes, 2); });
}

// y = conv(x, w) + bias; want_stats: *slab / *rows = the epilogue's [rows][3][Co] Welford rows
int dcnn_c_conv_fwd(const void* x, const void* w, const float* bias, void* y, const int* shape, int want_stats,
                    const float** slab, int* rows) {
  return guarded([&] {
    int r = 0;
    const float* s = gpu_ops::conv_fwd(x, w, bias, y, shape_of(shape), want_stats ? &r : nullptr);
    if (slab) *slab = s;
    if (rows) *rows = r;
  });
}

// dx = dgrad(dy, w) (+ residual); w_t: w is transposed here first and passed as the pre-transposed
// operand (the arena path); bnb: the fused BatchNorm backward (mask y_bn when non-null, statistics
// rows [rows][2][C] in *slab)
int dcnn_c_conv_dgrad(const void* dy, const void* w, int w_t, void* dx, const int* shape, const void* residual,
                      int bnb, const void* y_bn, const void* x_bn, const float* mean, const float* istd,
                      const float** slab, int* rows) {
  return guarded([&] {
    const ConvShape s = shape_of(shape);
    Tensor wt;
    const void* wop = w;
    if (w_t) {
      int dev = 0;
      wt = Tensor::empty({(int64_t)s.C * s.KH * s.KW * s.Co}, DType::BF16, Device::gpu(dev));
      gpu_ops::weight_transpose(w, wt.data(), s.Co, s.KH * s.KW, s.C);
      wop = wt.data();
    }
    gpu_ops::BnbOperands ops{y_bn, x_bn, mean, istd};
    int r = 0;
    const float* st = gpu_ops::conv_dgrad(dy, wop, dx, s, residual, w_t != 0, bnb ? &ops : nullptr, &r);
    if (slab) *slab = st;
    if (rows) *rows = r;
    gpu::synchronize();  // (wt is released after the kernels that read it)
  });
}

// dcnn_c_conv_dgrad (pre-transposed operand) with a phase-compact residual [N][H / SH][W / SW][C]
// (gpu_ops::DgradOpts::residual_compact); bnb as dcnn_c_conv_dgrad
int dcnn_c_conv_dgrad_compact_residual(const void* dy, const void* w, void* dx, const int* shape,
                                       const void* residual, int bnb, const void* y_bn, const void* x_bn,
                                       const float* mean, const float* istd, const float** slab, int* rows) {
  return guarded([&] {
    const ConvShape s = shape_of(shape);
    int dev = 0;
    Tensor wt = Tensor::empty({(int64_t)s.C * s.KH * s.KW * s.Co}, DType::BF16, Device::gpu(dev));
    gpu_ops::weight_transpose(w, wt.data(), s.Co, s.KH * s.KW, s.C);
    gpu_ops::BnbOperands ops{y_bn, x_bn, mean, istd};
    gpu_ops::DgradOpts opt;
    opt.residual_compact = true;
    int r = 0;
    const float* st = gpu_ops::conv_dgrad(dy, wt.data(), dx, s, residual, true, bnb ? &ops : nullptr, &r, opt);
    if (slab) *slab = st;
    if (rows) *rows = r;
    gpu::synchronize();  // (wt is released after the kernels that read it)
  });
}

// the [N][OH][OW][C] data gradient of a strided 1x1 pad-0 conv (gpu_ops::conv_dgrad_compact)
int dcnn_c_conv_dgrad_compact(const void* dy, const void* w, void* dxc, const int* shape) {
  return guarded([&] {
    const ConvShape s = shape_of(shape);
    int dev = 0;
    Tensor wt = Tensor::empty({(int64_t)s.C * s.KH * s.KW * s.Co}, DType::BF16, Device::gpu(dev));
    gpu_ops::weight_transpose(w, wt.data(), s.Co, s.KH * s.KW, s.C);
    gpu_ops::conv_dgrad_compact(dy, wt.data(), dxc, s, true);
    gpu::synchronize();
  });
}

int dcnn_c_conv_dgrad_takes_compact(const int* shape) { return gpu_ops::conv_dgrad_takes_compact(shape_of(shape)) ? 1 : 0; }

// gw / gb (+=) the weight / bias gradient; deferred: inside a backward's batched split-K reduce
int dcnn_c_conv_wgrad(const void* dy, const void* x, float* gw, float* gb, const int* shape, int deferred) {
  return guarded([&] {
    if (deferred) gpu_ops::begin_deferred_reduce();
    try {
      gpu_ops::conv_wgrad(dy, x, gw, gb, shape_of(shape));
    } catch (...) {
      if (deferred) gpu_ops::end_deferred_reduce();
      throw;
    }
    if (deferred) gpu_ops::end_deferred_reduce();
  });
}

// depthwise conv (shape[4] Co == shape[1] C): y = dwconv(x, w) + bias, w bf16 [C][KH][KW]
int dcnn_c_dwconv_fwd(const void* x, const void* w, const float* bias, void* y, const int* shape) {
  return guarded([&] { gpu_ops::dwconv_fwd(x, w, bias, y, shape_of(shape)); });
}

// dx = dwconv^T(dy, w) (+ residual)
int dcnn_c_dwconv_dgrad(const void* dy, const void* w, void* dx, const int* shape, const void* residual) {
  return guarded([&] { gpu_ops::dwconv_dgrad(dy, w, dx, shape_of(shape), residual); });
}

// gw / gb (+=) the weight / bias gradient; deferred: inside a backward's batched split-K reduce
int dcnn_c_dwconv_wgrad(const void* dy, const void* x, float* gw, float* gb, const int* shape, int deferred) {
  return guarded([&] {
    if (deferred) gpu_ops::begin_deferred_reduce();
    try {
      gpu_ops::dwconv_wgrad(dy, x, gw, gb, shape_of(shape));
    } catch (...) {
      if (deferred) gpu_ops::end_deferred_reduce();
      throw;
    }
    if (deferred) gpu_ops::end_deferred_reduce();
  });
}

// grouped conv (groups: the extra argument): y = gconv(x, w) + bias, w bf16 [Co][KH][KW][C / groups]
int dcnn_c_gconv_fwd(const void* x, const void* w, const float* bias, void* y, const int* shape, int groups) {
  return guarded([&] { gpu_ops::gconv_fwd(x, w, bias, y, shape_of(shape), groups); });
}

// dx = gconv^T(dy, w) (+ residual)
int dcnn_c_gconv_dgrad(const void* dy, const void* w, void* dx, const int* shape, int groups, const void* residual) {
  return guarded([&] { gpu_ops::gconv_dgrad(dy, w, dx, shape_of(shape), groups, residual); });
}

// gw / gb (+=) the weight / bias gradient; deferred: inside a backward's batched split-K reduce
int dcnn_c_gconv_wgrad(const void* dy, const void* x, float* gw, float* gb, const int* shape, int groups,
                       int deferred) {
  return guarded([&] {
    if (deferred) gpu_ops::begin_deferred_reduce();
    try {
      gpu_ops::gconv_wgrad(dy, x, gw, gb, shape_of(shape), groups);
    } catch (...) {
      if (deferred) gpu_ops::end_deferred_reduce();
      throw;
    }
    if (deferred) gpu_ops::end_deferred_reduce();
  });
}

int dcnn_c_stem_fwd(const float* x, const void* w, const float* bias, void* y, const int* shape, int want_stats,
                    const float** slab, int* rows) {
  return guarded([&] {
    int r = 0;
    const float* s = gpu_ops::stem_fwd(x, w, bias, y, shape_of(shape), want_stats ? &r : nullptr);
    if (slab) *slab = s;
    if (rows) *rows = r;
  });
}

int dcnn_c_stem_wgrad(const void* dy, const float* x, float* gw, float* gb, const int* shape, int deferred) {
  return guarded([&] {
    if (deferred) gpu_ops::begin_deferred_reduce();
    try {
      gpu_ops::stem_wgrad(dy, x, gw, gb, shape_of(shape));
    } catch (...) {
      if (deferred) gpu_ops::end_deferred_reduce();
      throw;
    }
    if (deferred) gpu_ops::end_deferred_reduce();
  });
}

// channel LayerNorm over bf16 NHWC rows [R][C]: y = (x - mean) rstd gamma + beta (gamma / beta null:
// no affine), mean / rstd fp32 [R] saved
int dcnn_c_layernorm_fwd(const void* x, void* y, long R, int C, const float* gamma, const float* beta, float eps,
                         float* mean, float* rstd) {
  return guarded([&] { gpu_ops::layernorm_fwd(x, y, R, C, gamma, beta, eps, mean, rstd); });
}

// dx of dcnn_c_layernorm_fwd; dgamma / dbeta (+=, may be null)
int dcnn_c_layernorm_bwd(const void* dy, const void* x, void* dx, long R, int C, const float* gamma, const float* mean,
                         const float* rstd, float* dgamma, float* dbeta) {
  return guarded([&] { gpu_ops::layernorm_bwd(dy, x, dx, R, C, gamma, mean, rstd, dgamma, dbeta); });
}

// LayerScale: y = gamma[c] x (+ residual)
int dcnn_c_layer_scale_fwd(const void* x, const float* gamma, const void* residual, void* y, long R, int C) {
  return guarded([&] { gpu_ops::layer_scale_fwd(x, gamma, residual, y, R, C); });
}

// dx = gamma[c] dy, dgamma (+=) the sum of dy x
int dcnn_c_layer_scale_bwd(const void* dy, const void* x, const float* gamma, void* dx, float* dgamma, long R, int C) {
  return guarded([&] { gpu_ops::layer_scale_bwd(dy, x, gamma, dx, dgamma, R, C); });
}

// Stochastic depth. The mask of (seed, draw): N floats, 0 or 1 / (1 - p), into the device buffer
// `mask` — the function the kernel module's and the native CPU module's drop_path_mask return.
int dcnn_c_drop_path_mask(float* mask, int N, float p, uint64_t seed, uint64_t draw) {
  return guarded([&] { gpu_ops::drop_path_mask(mask, N, p, seed, draw); });
}

// the same on the CPU backend, into a host buffer
int dcnn_c_drop_path_mask_host(float* mask, long N, float p, uint64_t seed, uint64_t draw) {
  try {
    cpu_ops::drop_path_mask(mask, N, p, seed, draw);
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  }
  return -1;
}

// Mixup / CutMix. The plan of training batch `step`: out6 = {mode, yl, yh, xl, xh, 0}, *lam = lam.
int dcnn_c_mix_plan(uint64_t seed, uint64_t step, int H, int W, double mixup_alpha, double cutmix_alpha, double prob,
                    double switch_prob, int* out6, double* lam) {
  try {
    const MixPlan p = cpu_ops::mix_plan(seed, step, H, W, mixup_alpha, cutmix_alpha, prob, switch_prob);
    out6[0] = p.mode; out6[1] = p.yl; out6[2] = p.yh; out6[3] = p.xl; out6[4] = p.xh; out6[5] = 0;
    *lam = p.lam;
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  }
  return -1;
}

// x fp32 [B][C][H][W] (device) mixed in place, target fp32 [B][K]; box = {yl, yh, xl, xh}
int dcnn_c_mix_batch(float* x, const int64_t* labels, float* target, long B, long C, long H, long W, int mode,
                     double lam, const int* box, long K) {
  return guarded([&] { gpu_ops::mix_batch(x, labels, target, B, C, H, W, mode, lam, box[0], box[1], box[2], box[3], K); });
}

// the same on the CPU backend, host pointers
int dcnn_c_mix_batch_host(float* x, const int64_t* labels, float* target, long B, long C, long H, long W, int mode,
                          double lam, const int* box, long K) {
  try {
    cpu_ops::mix_batch(x, labels, target, B, C, H, W, mode, lam, box[0], box[1], box[2], box[3], K);
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  }
  return -1;
}

// Soft-target cross entropy with label smoothing eps. Device: pred / grad bf16 [N][C], target fp32
// [N][C] or null with int64 labels; *loss the mean loss, *correct the argmax hits.
int dcnn_c_soft_loss(const void* pred, const float* target, const int64_t* labels, void* grad, int N, int C, float eps,
                     float grad_scale, double* loss, long* correct) {
  return guarded([&] { *loss = gpu_ops::loss(6, pred, target, labels, grad, N, C, eps, correct, grad_scale); });
}

// the same on the CPU backend: pred / grad fp32 host pointers
int dcnn_c_soft_loss_host(const float* pred, const float* target, const int64_t* labels, float* grad, long N, long C,
                          float eps, double* loss, long* correct) {
  try {
    *loss = cpu_ops::loss(6, pred, target, labels, grad, N, C, eps, correct);
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  }
  return -1;
}

// y[n][:] = mask[n] x[n][:] (+ residual[n][:]), bf16, samples of `row` elements
int dcnn_c_drop_path_scale(const void* x, const float* mask, const void* residual, void* y, long N, long row) {
  return guarded([&] { gpu_ops::drop_path_scale(x, mask, residual, y, N, row); });
}

// the drop tail: y = residual + mask[n] gamma[c] x; dx = mask[n] gamma[c] dy, dgamma (+=) sum mask[n] dy x
int dcnn_c_layer_scale_drop_fwd(const void* x, const float* gamma, const float* mask, const void* residual, void* y,
                                long R, int C, long rows_per_sample) {
  return guarded([&] { gpu_ops::layer_scale_drop_fwd(x, gamma, mask, residual, y, R, C, rows_per_sample); });
}

int dcnn_c_layer_scale_drop_bwd(const void* dy, const void* x, const float* gamma, const float* mask, void* dx,
                                float* dgamma, long R, int C, long rows_per_sample) {
  return guarded([&] { gpu_ops::layer_scale_drop_bwd(dy, x, gamma, mask, dx, dgamma, R, C, rows_per_sample); });
}

// Global-norm clipping and weight EMA over flat fp32 buffers. Device: out4 = {sumsq, norm, coef,
// max_norm}; the steps take optional inputs, null = off: nodecay (one byte per 64 elements), coef (a
// device pointer, e.g. out4 + 2; g itself is not rewritten), ema with its decay; shadow (bf16) may
// be null. hp = {lr, b1, b2, eps, bc1, bc2, wd} for Adam, {lr, momentum} for SGD.
int dcnn_c_grad_sumsq(const float* g, long n, float max_norm, float* out4) {
  return guarded([&] { gpu_ops::grad_sumsq(g, n, max_norm, out4); });
}

int dcnn_c_adam_tail(float* p, const float* g, float* m, float* v, void* shadow, long n, const float* hp, int decoupled,
                     const uint8_t* nodecay, const float* coef, float* ema, float decay) {
  return guarded([&] {
    gpu_ops::adam_tail(p, g, m, v, shadow, n, hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6], decoupled != 0, nullptr,
                       nodecay, coef, ema, decay);
  });
}

int dcnn_c_sgd_tail(float* p, const float* g, float* vel, void* shadow, long n, const float* hp, const float* coef,
                    float* ema, float decay) {
  return guarded([&] { gpu_ops::sgd_tail(p, g, vel, shadow, n, hp[0], hp[1], coef, ema, decay); });
}

int dcnn_c_ema_swap(float* a, float* b, void* shadow, long n) {
  return guarded([&] { gpu_ops::ema_swap(a, b, shadow, n); });
}

// Layer-wise optimizers (LAMB, LARS) over flat fp32 buffers. dcnn_c_optim_segments builds the
// segment / chunk tables from the slices (offsets / counts in elements, no_decay may be null, exclude:
// flagged slices neither adapt nor decay) as flat int32 rows: chunks [*nchunks][3] = {first 64-element
// block, blocks, segment}, segs [params][4] = {first chunk, chunks, adapt, decay}; *cover = the
// element the chunks reach. With chunks == null only *nchunks and *cover are written (size query);
// chunk_cap < *nchunks is an error. The device steps take the rows in device memory, part
// [2 nchunks] and out [3 nsegs] device floats (out: trust, then {sum p^2, sum u^2}); hyper / coef /
// ema optional. hp (doubles) = {lr, b1, b2, eps, bc1, bc2, wd} for LAMB, {lr, momentum, wd, tc, eps}
// for LARS. The _host steps take host rows and out [3 nsegs] doubles.
int dcnn_c_optim_segments(const long* offsets, const long* counts, const unsigned char* no_decay, int params,
                          int exclude, long n, int* chunks, int chunk_cap, int* segs, int* nchunks, long* cover) {
  try {
    const OptimSegments t = build_optim_segments(offsets, counts, no_decay, params, exclude != 0, n);
    *nchunks = (int)t.chunks.size();
    *cover = t.cover;
    if (!chunks) return 0;
    if (chunk_cap < *nchunks || !segs)
      throw std::invalid_argument("optim_segments: room for " + std::to_string(chunk_cap) + " chunk rows, " +
                                  std::to_string(*nchunks) + " needed (and segs is required)");
    for (size_t c = 0; c < t.chunks.size(); ++c) {
      chunks[3 * c] = t.chunks[c].first_block;
      chunks[3 * c + 1] = t.chunks[c].blocks;
      chunks[3 * c + 2] = t.chunks[c].segment;
    }
    for (size_t k = 0; k < t.segs.size(); ++k) {
      segs[4 * k] = t.segs[k].first_chunk;
      segs[4 * k + 1] = t.segs[k].chunks;
      segs[4 * k + 2] = t.segs[k].adapt;
      segs[4 * k + 3] = t.segs[k].decay;
    }
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  }
  return -1;
}

int dcnn_c_lamb_step(float* p, const float* g, float* m, float* v, void* shadow, long n, const double* hp,
                     const float* hyper, const float* coef, float* ema, float decay, const void* chunks, int nchunks,
                     const void* segs, int nsegs, long cover, float* part, float* out) {
  return guarded([&] {
    gpu_ops::lamb(p, g, m, v, shadow, n, (float)hp[0], hp[1], hp[2], (float)hp[3], (float)hp[4], (float)hp[5],
                  (float)hp[6], hyper, coef, ema, decay, chunks, nchunks, segs, nsegs, cover, part, out);
  });
}

int dcnn_c_lars_step(float* p, const float* g, float* vel, void* shadow, long n, const double* hp, const float* hyper,
                     const float* coef, float* ema, float decay, const void* chunks, int nchunks, const void* segs,
                     int nsegs, long cover, float* part, float* out) {
  return guarded([&] {
    gpu_ops::lars(p, g, vel, shadow, n, (float)hp[0], (float)hp[1], (float)hp[2], (float)hp[3], (float)hp[4], hyper,
                  coef, ema, decay, chunks, nchunks, segs, nsegs, cover, part, out);
  });
}

int dcnn_c_lamb_step_host(float* p, const float* g, float* m, float* v, long n, const double* hp, const double* coef,
                          float* ema, float decay, const int* chunks, int nchunks, const int* segs, int nsegs,
                          double* out) {
  try {
    check_optim_segments(reinterpret_cast<const SegChunk*>(chunks), nchunks, reinterpret_cast<const SegInfo*>(segs),
                         nsegs, (n + kSegBlock - 1) / kSegBlock * kSegBlock);
    cpu_ops::lamb(p, g, m, v, n, (float)hp[0], hp[1], hp[2], (float)hp[3], hp[4], hp[5], (float)hp[6], coef, ema, decay,
                  chunks, nchunks, segs, nsegs, out);
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  }
  return -1;
}

int dcnn_c_lars_step_host(float* p, const float* g, float* vel, long n, const double* hp, const double* coef, float* ema,
                          float decay, const int* chunks, int nchunks, const int* segs, int nsegs, double* out) {
  try {
    check_optim_segments(reinterpret_cast<const SegChunk*>(chunks), nchunks, reinterpret_cast<const SegInfo*>(segs),
                         nsegs, (n + kSegBlock - 1) / kSegBlock * kSegBlock);
    cpu_ops::lars(p, g, vel, n, (float)hp[0], (float)hp[1], (float)hp[2], (float)hp[3], (float)hp[4], coef, ema, decay,
                  chunks, nchunks, segs, nsegs, out);
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  }
  return -1;
}

// the same on the CPU backend, host pointers: *sumsq the sum of g^2; coef null = no clipping
int dcnn_c_grad_sumsq_host(const float* g, long n, double* sumsq) {
  try {
    *sumsq = cpu_ops::grad_sumsq(g, n);
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  }
  return -1;
}

int dcnn_c_adam_tail_host(float* p, const float* g, float* m, float* v, long n, const float* hp, int decoupled,
                          const uint8_t* nodecay, const double* coef, float* ema, float decay) {
  try {
    cpu_ops::adam_tail(p, g, m, v, n, hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6], decoupled != 0, nodecay, coef,
                       ema, decay);
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  }
  return -1;
}

int dcnn_c_sgd_tail_host(float* p, const float* g, float* vel, long n, const float* hp, const double* coef, float* ema,
                         float decay) {
  try {
    cpu_ops::sgd_tail(p, g, vel, n, hp[0], hp[1], coef, ema, decay);
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  }
  return -1;
}

int dcnn_c_ema_swap_host(float* a, float* b, long n) {
  try {
    cpu_ops::ema_swap(a, b, n);
    return 0;
  } catch (const std::exception& e) {
    t_err = e.what();
  }
  return -1;
}

}  // extern "C"
