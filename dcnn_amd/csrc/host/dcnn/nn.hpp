// C++ host API: layers, Sequential / SequentialBuilder, loss, optimizers, training loop.
//
// A C++ program builds, trains, saves and reloads a model without Python:
//
//   auto model = dcnn::SequentialBuilder("mnist_cnn").input({1, 28, 28})
//                    .conv2d(16, 3, 3, 1, 1, 1, 1).batchnorm().activation("relu").maxpool2d(2, 2)
//                    .flatten().dense(10).build();
//   model.set_device(dcnn::Device::gpu(0));
//   model.initialize(42);
//   dcnn::Adam opt(1e-3f);
//   dcnn::train_classification_model(model, train_source, &test_source, opt, cfg);
//   model.save_to_file("snapshots/mnist_cnn");   // path.json + path.bin, readable by Python
//
// CPU: fp32 NCHW on the native CPU kernels. GPU: bf16 NHWC activations on the HIP/CDNA4 kernel
// library with fp32 master parameters (Adam / SGD write the bf16 operand shadows in the same
// kernel). The architecture JSON and the .bin weight records are the formats of the Python front
// end (dcnn_amd/nn/sequential.py) and of the reference, so a model moves between the two.
// Reference parity: include/nn/sequential.hpp:39-1340 (Sequential, SequentialBuilder),
// include/nn/train.hpp:202 (train_classification_model), include/nn/optimizers.hpp,
// include/nn/loss.hpp, examples/mnist_cnn_trainer.cpp.
#pragma once
#include <cmath>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "json.hpp"
#include "ops.hpp"
#include "tensor.hpp"

namespace dcnn {

// One trainable tensor. `value` / `grad` are fp32 on the layer's device in `layout` (GPU conv
// weights: physical [Co][KH][KW][Ci] = NHWC of the logical (Co, Ci, KH, KW)); `shadow` is the bf16
// GEMM operand copy on the GPU. `shape` is the logical 4-D shape of the .bin record.
struct ParamArena;
struct OptimSegments;  // csrc/kernels/optim_segments.h: the layer-wise optimizers' segment / chunk tables
struct Param {
  std::string name;
  std::vector<int64_t> shape;
  Layout layout = Layout::NCHW;
  Tensor value, grad, shadow;
  Tensor m, v;  // optimizer state (lazily created)
  Tensor ema;   // weight EMA of the per-parameter path (an optimizer with set_ema_decay; lazily created)
  // excluded from weight decay when the optimizer's no_decay_norm_bias is on: set by the owning
  // layer for biases, norm affines and layer scales (by kind, never by shape)
  bool no_decay = false;
  std::shared_ptr<ParamArena> arena;  // GPU: the flat buffers value / grad / m / v / shadow live in
};

// GPU parameter arena of a Sequential: every parameter's value, gradient, optimizer moments and
// bf16 shadow as slices of five flat buffers (64-element aligned), so zero_grad is one memset and
// an optimizer step one fused kernel over all `count` parameters (`n` elements, gaps stay zero)
struct ParamArena {
  Tensor value, grad, m, v, shadow;
  size_t n = 0, count = 0;
  // one byte per 64-element block, 1 where the block belongs to a Param with no_decay (built once
  // by Sequential::pack_params: static, so a captured optimizer step replays it as it is)
  Tensor nodecay;
  // weight EMA (an optimizer with set_ema_decay): a flat buffer of n floats, a copy of `value` when
  // it is created, updated inside the fused step; undefined while the EMA is off
  Tensor ema;
  // layer-wise optimizers (LAMB, LARS): one segment per parameter, chunks of at most 4096 elements
  // (built once by Sequential::pack_params with the kernel library's shared builder: static, so a
  // captured step replays them as they are). segments[0]: every parameter adapts and decays;
  // segments[1]: the Param::no_decay ones do neither. The chunk rows are the same for both.
  std::shared_ptr<const OptimSegments> segments[2];
  Tensor seg_chunks, seg_info[2];  // the device rows
  // every eligible conv's dgrad operand ([C][KH][KW][Co] bf16), regenerated from the shadows in
  // one batched launch after each fused optimizer step (rows: src, dst, Co, T, C)
  Tensor wt_table;
  int n_wt = 0;
  long wt_tiles = 0;
  bool wt_valid = false;
  void refresh_transposes();
};

class Layer {
 public:
  explicit Layer(std::string name) : name_(std::move(name)) {}
  virtual ~Layer() = default;
  virtual std::string type() const = 0;
  virtual json::Value parameters_config() const = 0;
  // logical (N, C, H, W) output shape for a logical input shape
  virtual std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const = 0;
  // create parameters for the given input shape on `dev` (deterministic in `seed`)
  virtual void build(const std::vector<int64_t>& in, Device dev, uint64_t seed) { (void)in; (void)seed; dev_ = dev; }
  virtual Tensor forward(const Tensor& x, bool training) = 0;
  virtual Tensor backward(const Tensor& dy) = 0;
  // refresh the bf16 operand shadows from the fp32 masters (after loading weights)
  virtual void sync_shadow();
  // this layer's parameters, then those of its sub-layers (ResidualBlock), in checkpoint order
  virtual void collect_params(std::vector<Param*>& out) {
    for (auto& p : params_) out.push_back(&p);
  }
  // this layer and, depth-first, every sub-layer (BatchNorm statistics sidecar order)
  virtual void collect_layers(std::vector<Layer*>& out) { out.push_back(this); }
  std::vector<Param>& params() { return params_; }
  const std::string& name() const { return name_; }
  Device device() const { return dev_; }
  // micro-batch whose forward state the next forward / backward call uses: every layer keeps its
  // forward caches per micro-batch (the reference's unordered_map<size_t, ...> caches), so a
  // pipeline stage can hold several micro-batches in flight (semi-async, 1F1B)
  virtual void set_micro_batch(int mb) { mb_ = mb; }
  void clear_caches() { caches_.clear(); }
  // false: backward need not produce the input gradient (the network's first layer); the layers
  // that can skip their data-gradient GEMM (Conv2D, Dense) then return an undefined tensor
  void set_input_grad(bool b) { input_grad_ = b; }
  bool input_grad() const { return input_grad_; }
  // the network input (fp32 NCHW, logical input shape `in`) is consumed as is (GPU RGB stem conv)
  virtual bool takes_raw_input(const std::vector<int64_t>& in) const { (void)in; return false; }
  // forward + backward FLOPs for a logical input shape (the pipeline's FLOP-balanced partition;
  // the Python layers' forward_flops + backward_flops)
  virtual double flops(const std::vector<int64_t>& in) const { (void)in; return 0; }

 protected:
  struct MbCache {
    Tensor a, b, c, d;
    std::vector<int64_t> shape;
    uint64_t u = 0;
    bool flag = false;
  };
  MbCache& mbc() { return caches_[mb_]; }
  std::map<int, MbCache> caches_;
  int mb_ = 0;
  bool input_grad_ = true;
  Param& add_param(const std::string& n, const std::vector<int64_t>& shape, Layout phys, const std::vector<float>& init);
  std::string name_;
  Device dev_ = Device::cpu();
  std::vector<Param> params_;
};

// What a 2-D convolution layer's geometry and parameters are, once for the three conv layers:
// weights (Co, Ci / G, KH, KW) and an optional bias (Co), dense G == 1, depthwise Ci == Co == G.
// forward / backward here are the depthwise and grouped passes (they differ in the gpu_ops /
// cpu_ops entry only, chosen by depthwise()); Conv2D overrides both.
class ConvBase : public Layer {
 public:
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override;
  void build(const std::vector<int64_t>& in, Device dev, uint64_t seed) override;
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override { return backward_impl(dy, nullptr); }
  double flops(const std::vector<int64_t>& in) const override;
  // GPU: backward whose input gradient also adds `residual` in the data-gradient epilogue (the
  // shortcut gradient of a block whose main path starts with this layer), into dx; false: the
  // layer has no such fusion (the caller runs backward and adds)
  virtual bool backward_residual(const Tensor& dy, const Tensor& residual, Tensor& dx) {
    (void)dy; (void)residual; (void)dx;
    return false;
  }
  int stride_h() const { return sh_; }
  int stride_w() const { return sw_; }

 protected:
  ConvBase(int in_ch, int out_ch, int kh, int kw, int groups, int sh, int sw, int ph, int pw, bool bias,
           std::string name)
      : Layer(std::move(name)), ci_(in_ch), co_(out_ch), kh_(kh), kw_(kw), g_(groups), sh_(sh), sw_(sw), ph_(ph),
        pw_(pw), bias_(bias) {}
  ConvShape shape_for(const std::vector<int64_t>& in) const;
  // stride_h .. use_bias into `p`, after the subclass's channel and kernel keys (the saved key order)
  void geometry_config(json::Value& p) const;
  const float* bias_value() const { return bias_ ? params_[1].value.ptr<float>() : nullptr; }
  float* bias_grad() { return bias_ ? params_[1].grad.ptr<float>() : nullptr; }
  // the dwconv kernels and their weight layout ([C][KH][KW] on every device): DepthwiseConv2D
  virtual bool depthwise() const { return false; }
  int group_in() const { return depthwise() ? 1 : ci_ / g_; }  // Ci / G
  Tensor backward_impl(const Tensor& dy, const Tensor* residual);
  int ci_, co_, kh_, kw_, g_, sh_, sw_, ph_, pw_;
  bool bias_;
};

class Conv2D : public ConvBase {
 public:
  Conv2D(int in_ch, int out_ch, int kh, int kw, int sh = 1, int sw = 1, int ph = 0, int pw = 0, bool bias = true,
         std::string name = "conv2d");
  std::string type() const override { return "conv2d"; }
  json::Value parameters_config() const override;
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override;
  bool takes_raw_input(const std::vector<int64_t>& in) const override;
  // GPU: hand the output's BatchNorm statistics, computed in the conv epilogue, to `bn` (the
  // BatchNorm that consumes this conv's output; fuse_bn_relu wires it)
  void set_stats_consumer(class BatchNorm* bn) { stats_to_ = bn; }
  // GPU: the BatchNorm (+ ReLU) producing this conv's input; the data gradient's epilogue applies
  // its ReLU mask and computes its backward statistics (fuse_bn_relu wires it)
  void set_bnb_producer(class BatchNorm* bn) { bnb_from_ = bn; }
  // the same across a residual-block boundary: the previous block's tail BatchNorm (its mask is
  // the block output), applied only by backward_residual (after the shortcut gradient is added)
  void set_block_bnb_producer(class BatchNorm* bn) { bnb_block_from_ = bn; }
  bool backward_residual(const Tensor& dy, const Tensor& residual, Tensor& dx) override;
  // GPU, a downsample block's pair (ResidualBlock::backward). The shortcut's side: this 1x1 pad-0
  // strided conv's data gradient only reaches the pixels (SH i, SW j), and backward_compact returns
  // just those, (N, Ci, H / SH, W / SW), with the weight gradient as backward runs it. The head
  // conv's side: backward_residual takes that tensor as `residual` when takes_compact_residual
  // (same strides; its data gradient on the stride-phase-grouped gemm_g2 launch)
  bool compact_grad_ok() const;
  Tensor backward_compact(const Tensor& dy);
  bool takes_compact_residual(int sh, int sw) const;
  // GPU RGB stem (the network input, fp32, on the stem kernel): true when this micro-batch's
  // forward ran it, so backward_stem_bn applies
  bool ran_stem() const;
  // the stem's weight gradient with its BatchNorm's backward applied to `dy` on the fly
  // (Sequential::backward_activation; gpu_ops::stem_wgrad_bn)
  void backward_stem_bn(const Tensor& dy, const gpu_ops::StemBn& bn);
  void sync_shadow() override;
  // GPU parameter arena: allocate this conv's pre-transposed dgrad operand; the arena's batched
  // transpose row and tile count (false: not eligible)
  bool make_transposed_operand(std::vector<int64_t>& row, long& tiles);

 private:
  class BatchNorm* stats_to_ = nullptr;
  class BatchNorm* bnb_from_ = nullptr;
  class BatchNorm* bnb_block_from_ = nullptr;
  Tensor wt_;  // pre-transposed dgrad operand (arena-managed)
  const void* dgrad_operand(bool& transposed) const;
};

// Depthwise convolution (groups = C, channel multiplier 1): weights (C, 1, KH, KW), NCHW and NHWC
// the same bytes [C][KH][KW]. Shares ConvBase; not a Conv2D for the planner: it sees FK_OTHER (no
// statistics epilogue, no backward-BatchNorm fusion, no transposed operand); the BatchNorm around
// it runs its own statistics passes.
class DepthwiseConv2D : public ConvBase {
 public:
  DepthwiseConv2D(int channels, int kh, int kw, int sh = 1, int sw = 1, int ph = 0, int pw = 0, bool bias = true,
                  std::string name = "depthwise_conv2d");
  std::string type() const override { return "depthwise_conv2d"; }
  json::Value parameters_config() const override;
  // dx = conv^T(dy) + residual (GPU): wgrad + the fused data gradient
  bool backward_residual(const Tensor& dy, const Tensor& residual, Tensor& dx) override;

 protected:
  bool depthwise() const override { return true; }
};

// Grouped convolution (1 < groups < channels): weights (Co, Ci / G, KH, KW). Shares ConvBase; not
// a Conv2D for the planner: it sees FK_OTHER (no statistics epilogue, no backward-BatchNorm
// fusion); the data gradient can add a residual (the shortcut gradient of a block whose main path
// starts with it) in its store.
class GroupedConv2D : public ConvBase {
 public:
  GroupedConv2D(int in_ch, int out_ch, int kh, int kw, int groups, int sh = 1, int sw = 1, int ph = 0, int pw = 0,
                bool bias = true, std::string name = "grouped_conv2d");
  std::string type() const override { return "grouped_conv2d"; }
  json::Value parameters_config() const override;
  // dx = conv^T(dy) + residual (GPU): wgrad + the fused data gradient
  bool backward_residual(const Tensor& dy, const Tensor& residual, Tensor& dx) override;
};

class Dense : public Layer {
 public:
  Dense(int in_features, int out_features, bool bias = true, std::string name = "dense");
  std::string type() const override { return "dense"; }
  json::Value parameters_config() const override;
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override;
  void build(const std::vector<int64_t>& in, Device dev, uint64_t seed) override;
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override;
  double flops(const std::vector<int64_t>& in) const override { return 6.0 * in[0] * in_ * out_; }
  // GPU classifier head (average pool -> flatten -> dense closing a sequence; fuse_bn_relu wires
  // it): the pool's training forward runs gpu_ops::head_fwd, pool + this layer in one kernel, and
  // hands the pooled tile (this layer's cached input) and the logits over (run_head); forward then
  // returns those logits, and backward runs gpu_ops::head_bwd and returns the pool's input
  // gradient, which the flatten and the pool recognise and pass through (is_head_dx). Each
  // hand-over is by tensor identity, so a layer driven on its own (a teacher-forced segment)
  // runs its own kernels.
  void set_head_pool(class Pool2D* p) { head_pool_ = p; }
  // false: geometry outside gpu_ops::head_supported (the pool runs its own kernel)
  bool run_head(const Tensor& x, const PoolShape& p, Tensor& pooled);
  // dy is the pool's input gradient this layer's backward just computed; take: the last consumer
  bool is_head_dx(const Tensor& dy, bool take);

 private:
  int in_, out_;
  bool bias_;
  class Pool2D* head_pool_ = nullptr;
};

class BatchNorm : public Layer {
 public:
  explicit BatchNorm(int num_features, float eps = 1e-5f, float momentum = 0.1f, bool affine = true,
                     std::string name = "batchnorm");
  std::string type() const override { return "batchnorm"; }
  json::Value parameters_config() const override;
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override { return in; }
  double flops(const std::vector<int64_t>& in) const override {
    return 15.0 * (double)in[0] * (double)in[1] * (double)in[2] * (double)in[3];  // 6 forward + 9 backward
  }
  void build(const std::vector<int64_t>& in, Device dev, uint64_t seed) override;
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override;
  // GPU: the following ReLU runs inside this layer's apply / backward kernels (fuse_bn_relu)
  void set_fused_relu(bool b) { fused_relu_ = b; }
  bool fused_relu() const { return fused_relu_; }
  // GPU: y = act(bn(x) + residual) in one pass (a residual block's tail BatchNorm, act = ReLU when
  // `relu`), and its backward: the BatchNorm input gradient, *branch = the (masked) dy the
  // shortcut branch receives
  Tensor forward_residual(const Tensor& x, const Tensor& residual, bool relu, bool training);
  Tensor backward_residual(const Tensor& dy, Tensor* branch);
  // GPU pairing with a projection shortcut's BatchNorm (`deferred`): forward_deferred takes that
  // layer's statistics rows now; the tail's forward_dual applies both BatchNorms, the residual add
  // and the activation in one pass. backward_dual: both data gradients from one pass over the
  // tail's masked gradient (false: not applicable, the caller runs the two backwards)
  void forward_deferred(const Tensor& x, bool training);
  Tensor forward_dual(const Tensor& x, BatchNorm& deferred, bool relu, bool training);
  bool backward_dual(const Tensor& dy, BatchNorm& deferred, Tensor& dx, Tensor& dx_deferred);
  // GPU: the following ReLU + max-pool run inside this layer's training apply (fuse_bn_relu; the
  // stem's BatchNorm -> ReLU -> max-pool)
  void set_fused_pool(class Pool2D* p) { fused_pool_ = p; }
  bool fused_pool() const { return fused_pool_ != nullptr; }
  // backward-fusion operands of micro-batch `mb` (its forward's input, output mask, statistics)
  gpu_ops::BnbOperands bnb_operands(int mb);
  // the next backward over the gradient at `dy` takes its statistics from this consumer slab (the
  // gradient is already masked)
  void offer_bwd_stats(const void* dy, const float* slab, int rows) {
    bwd_dy_ = dy;
    bwd_slab_ = slab;
    bwd_rows_ = rows;
  }
  // the next forward over the tensor at `x` takes its statistics from this producer slab
  void offer_stats(const void* x, const float* slab, int rows) {
    pending_x_ = x;
    pending_slab_ = slab;
    pending_rows_ = rows;
  }
  // GPU: this layer's backward over `dy` folded into the stem conv's weight gradient (its input
  // gradient has no other consumer): false when not applicable (no consumer statistics slab for
  // dy, or eval mode), the caller then runs the two backwards
  bool backward_into_stem(const Tensor& dy, Conv2D& stem);
  Tensor running_mean, running_var;

 private:
  int c_;
  float eps_, momentum_;
  bool affine_;
  bool train_ = true;
  bool fused_relu_ = false;
  Tensor forward_impl(const Tensor& x, bool training, const Tensor* residual, bool relu);
  Tensor apply_deferred(bool training);
  class Pool2D* fused_pool_ = nullptr;
  gpu_ops::BnRaw deferred_raw_{nullptr, 0};
  const void* bwd_dy_ = nullptr;
  const float* bwd_slab_ = nullptr;
  int bwd_rows_ = 0;
  const void* pending_x_ = nullptr;
  const float* pending_slab_ = nullptr;
  int pending_rows_ = 0;
};

// activation kinds: relu, leaky_relu (0.01), elu (alpha 1), sigmoid, tanh, linear, softmax (over the
// channels of every pixel)
class Activation : public Layer {
 public:
  explicit Activation(std::string kind = "relu", std::string name = "activation");
  std::string type() const override { return "activation"; }
  json::Value parameters_config() const override;
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override { return in; }
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override;
  bool is_relu() const;
  // GPU: the preceding BatchNorm applies this ReLU (fuse_bn_relu); forward / backward pass through
  void set_passthrough(bool b) { passthrough_ = b; }

 private:
  std::string kind_;
  int code_;
  bool passthrough_ = false;
};

// GroupNorm over G channel groups per image; gamma / beta per channel
// (reference include/nn/layers_impl/groupnorm_layer.tpp:21-321)
class GroupNorm : public Layer {
 public:
  GroupNorm(int num_groups, int num_channels, float eps = 1e-5f, bool affine = true, std::string name = "groupnorm");
  std::string type() const override { return "groupnorm"; }
  json::Value parameters_config() const override;
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override { return in; }
  void build(const std::vector<int64_t>& in, Device dev, uint64_t seed) override;
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override;

 private:
  int g_, c_;
  float eps_;
  bool affine_;
  bool gb_identity_ = false;
  Tensor ident_, scratch_;
};

// Channel LayerNorm: every (n, h, w) position over its C channels (F.layer_norm over the channel
// dimension; not GroupNorm(1, C), which normalises over C H W); gamma / beta per channel. GPU:
// lnorm.hip. No reference counterpart.
class LayerNorm : public Layer {
 public:
  explicit LayerNorm(int num_channels, float eps = 1e-6f, bool affine = true, std::string name = "layernorm");
  std::string type() const override { return "layernorm"; }
  json::Value parameters_config() const override;
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override { return in; }
  void build(const std::vector<int64_t>& in, Device dev, uint64_t seed) override;
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override;

 private:
  int c_;
  float eps_;
  bool affine_;
};

// Learnable per-channel scale y = gamma[c] x (a ConvNeXt block's layer scale). Closing the main
// path of an identity-shortcut block without activation it also adds the block input in its store
// (forward_residual: ResidualBlock::scale_tail).
class LayerScale : public Layer {
 public:
  explicit LayerScale(int num_channels, float init_value = 1e-6f, std::string name = "layer_scale");
  std::string type() const override { return "layer_scale"; }
  json::Value parameters_config() const override;
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override { return in; }
  void build(const std::vector<int64_t>& in, Device dev, uint64_t seed) override;
  Tensor forward(const Tensor& x, bool training) override { return forward_residual(x, nullptr, training); }
  // gamma x + residual; with `mask` (fp32 [N], a DropPath's: GPU only) mask[n] gamma x + residual,
  // and the backward applies the same mask
  Tensor forward_residual(const Tensor& x, const Tensor* residual, bool training, const Tensor* mask = nullptr);
  Tensor backward(const Tensor& dy) override;

 private:
  int c_;
  float init_;
};

// Stochastic depth: in training every sample n is scaled by m[n], 0 with probability `rate` and
// 1 / (1 - rate) otherwise, forward and backward; identity in eval or at rate 0. m is one function
// of (seed, draw, n) (cpu_ops / gpu_ops drop_path_mask, the Python front end's DropPath draws the
// same floats): draw counts this layer's training forwards from 1; the seed is the explicit one
// when given (then part of the JSON config), else the one build() derives. GPU: the mask lives in
// a per-micro-batch device buffer written once per forward, and the draw index in a device word
// bumped in-stream, so a replayed TrainGraph draws a new mask each time. Closing a residual block
// behind a LayerScale, the LayerScale's store applies the mask (ResidualBlock::drop_tail).
class DropPath : public Layer {
 public:
  explicit DropPath(float rate, std::string name = "drop_path", bool has_seed = false, uint64_t seed = 0);
  std::string type() const override { return "drop_path"; }
  json::Value parameters_config() const override;
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override { return in; }
  double flops(const std::vector<int64_t>& in) const override;
  void build(const std::vector<int64_t>& in, Device dev, uint64_t seed) override;
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override;
  float rate() const { return p_; }
  uint64_t mask_seed() const { return has_seed_ ? explicit_seed_ : seed_; }
  // draw the next mask for N samples into the current micro-batch's buffer; nullptr when the layer
  // is the identity (eval, rate 0). forward and a block's drop tail call it.
  const Tensor* draw_mask(int64_t N, bool training);
  // the last mask of the current micro-batch (fp32 [N], on the layer's device)
  const Tensor& last_mask() { return mbc().a; }
  // GPU: the device draw counter (a step runner that rolls warm-up steps back rolls it back too)
  Tensor& draw_counter() { return ctr_; }

 private:
  float p_;
  bool has_seed_;
  uint64_t explicit_seed_, seed_ = 0, draws_ = 0;
  Tensor ctr_;
};

// inverted dropout (scale 1 / (1 - p)), identity in eval; the mask is a counter-based function
// of (seed, element), regenerated in backward (reference include/nn/layers_impl/dropout_layer.tpp)
class Dropout : public Layer {
 public:
  explicit Dropout(float rate = 0.5f, std::string name = "dropout");
  std::string type() const override { return "dropout"; }
  json::Value parameters_config() const override;
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override { return in; }
  void build(const std::vector<int64_t>& in, Device dev, uint64_t seed) override;
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override;

 private:
  float p_;
  uint64_t seed_ = 0, draw_ = 0;
};

class Pool2D : public Layer {
 public:
  Pool2D(bool max, int kh, int kw, int sh, int sw, int ph, int pw, std::string name);
  std::string type() const override { return max_ ? "maxpool2d" : "avgpool2d"; }
  json::Value parameters_config() const override;
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override;
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override;
  bool is_max() const { return max_; }
  PoolShape shape_for(const std::vector<int64_t>& in) const;
  // GPU: the preceding BatchNorm + ReLU computes this pool's output in its training apply
  // (BatchNorm::set_fused_pool); forward then passes it through and backward is the max-pool
  // backward fused with that BatchNorm's backward statistics
  void set_fused_producer(class BatchNorm* bn) { bn_ = bn; }
  // the index buffer for a pre-pooled output `ypool` of an input of shape `in`
  uint8_t* accept_prepooled(const Tensor& ypool, const std::vector<int64_t>& in);
  void clear_prepooled() { mbc().flag = false; }
  // GPU: this average pool opens the classifier head that `d` closes (Dense::set_head_pool)
  void set_head_dense(class Dense* d) { head_ = d; }

 private:
  class BatchNorm* bn_ = nullptr;
  class Dense* head_ = nullptr;
  bool max_;
  int kh_, kw_, sh_, sw_, ph_, pw_;
};

class Flatten : public Layer {
 public:
  explicit Flatten(std::string name = "flatten") : Layer(std::move(name)) {}
  std::string type() const override { return "flatten"; }
  json::Value parameters_config() const override { return json::Value::object(); }
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override;
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override;
  // GPU: between the pool and the dense layer of a fused classifier head (Dense::set_head_pool)
  void set_head_dense(class Dense* d) { head_ = d; }

 private:
  class Dense* head_ = nullptr;
};

// out = act(F(x) + S(x)): F the main path, S the projection shortcut (identity when empty).
// Backward sums the main and shortcut input gradients. Config: sub-layer records as JSON strings
// ("main_path", "shortcut_path"), as the Python front end and the reference write them
// (include/nn/blocks_impl/residual_block.hpp:30-476).
class ResidualBlock : public Layer {
 public:
  ResidualBlock(std::vector<std::unique_ptr<Layer>> main, std::vector<std::unique_ptr<Layer>> shortcut,
                std::string activation = "relu", std::string name = "residual_block");
  std::string type() const override { return "residual_block"; }
  json::Value parameters_config() const override;
  std::vector<int64_t> output_shape(const std::vector<int64_t>& in) const override;
  double flops(const std::vector<int64_t>& in) const override;
  void build(const std::vector<int64_t>& in, Device dev, uint64_t seed) override;
  Tensor forward(const Tensor& x, bool training) override;
  Tensor backward(const Tensor& dy) override;
  void sync_shadow() override;
  void collect_params(std::vector<Param*>& out) override;
  void collect_layers(std::vector<Layer*>& out) override;
  void set_micro_batch(int mb) override;
  const std::vector<std::unique_ptr<Layer>>& main_path() const { return main_; }
  const std::vector<std::unique_ptr<Layer>>& shortcut_path() const { return short_; }
  // GPU: the main path's tail BatchNorm adds the shortcut and applies the block activation
  class BatchNorm* fused_tail() const;
  // the main path's first layer when it is a conv (its dgrad adds the shortcut gradient)
  class Conv2D* head_conv() const;
  // GPU: the projection shortcut's closing BatchNorm, paired with the fused tail
  // (BatchNorm::forward_dual / backward_dual); null without one
  class BatchNorm* dual_shortcut() const;
  // GPU: the main path's closing LayerScale of an identity-shortcut block without activation: its
  // store adds the block input, the first layer's data gradient adds the shortcut gradient
  class LayerScale* scale_tail() const;
  // GPU: the DropPath behind that LayerScale (main path closing in LayerScale, DropPath:
  // RF_DROP_TAIL), whose mask the LayerScale's store applies; null without one
  class DropPath* drop_tail() const;

 private:
  std::vector<std::unique_ptr<Layer>> main_, short_;
  std::string act_;
};

// layer from its JSON record {"type", "name", "parameters"} (the LayerFactory of the formats)
std::unique_ptr<Layer> create_layer(const json::Value& rec);

// GPU fusion pass over a layer sequence: every BatchNorm directly followed by a ReLU applies the
// ReLU itself (one pass instead of two forward and backward; the ReLU layer passes through), and
// every conv directly followed by a BatchNorm hands it the statistics its epilogue computed (no
// statistics pass over the conv output). `on` false undoes it (CPU placement).
// Sequential::initialize / ResidualBlock::build run it.
void fuse_bn_relu(std::vector<std::unique_ptr<Layer>>& seq, bool on);
// after the layers are built: consecutive residual blocks with fused tails — the next block's
// head-conv data gradient (shortcut gradient added) also masks with the previous block's output
// and computes its tail BatchNorm's backward statistics
void fuse_blocks(std::vector<std::unique_ptr<Layer>>& seq, bool on);

class Sequential {
 public:
  explicit Sequential(std::string name = "sequential") : name_(std::move(name)) {}
  Sequential(Sequential&&) = default;
  Sequential& operator=(Sequential&&) = default;
  void add(std::unique_ptr<Layer> l) { layers_.push_back(std::move(l)); }
  void set_input_shape(const std::vector<int64_t>& chw) { input_chw_ = chw; }
  void set_device(Device d);
  Device device() const { return dev_; }
  void initialize(uint64_t seed = 0);
  void set_training(bool t) { training_ = t; }
  bool is_training() const { return training_; }
  // x: fp32 logical NCHW (host or device); returns the logits [N, classes] as a device tensor
  Tensor forward(const Tensor& x, int mb = 0);
  void backward(const Tensor& dlogits, int mb = 0);
  // one partition of a pipeline: activations in the device layout in and out (GPU: bf16 NHWC,
  // CPU: fp32 NCHW); backward returns the input gradient in the same layout
  Tensor forward_activation(const Tensor& x, int mb);
  Tensor backward_activation(const Tensor& g, int mb);
  // the network input (fp32 NCHW, any device) as the first layer's activation
  Tensor input_activation(const Tensor& x) const;
  std::vector<Param*> parameters();
  // forward + backward FLOPs of every top-level layer for an (N, C, H, W) input
  std::vector<double> layer_flops(const std::vector<int64_t>& in) const;
  // every BatchNorm, depth-first through residual blocks (the .bnstats record order)
  std::vector<BatchNorm*> batchnorms();
  void zero_grad();
  size_t num_parameters();
  const std::vector<std::unique_ptr<Layer>>& layers() const { return layers_; }
  const std::string& name() const { return name_; }
  // called with the top-level layer index after each layer's backward (in backward order), inside
  // a capture too (the data-parallel bucket all-reduces start from here: dist::DataParallel)
  void set_backward_hook(std::function<void(size_t)> f) { bwd_hook_ = std::move(f); }

  json::Value get_config() const;
  void print_config() const;
  static Sequential load_from_config(const json::Value& cfg);
  // path.json (architecture) + path.bin (parameters in layer order, logical NCHW fp32) +
  // path.bnstats (BatchNorm running statistics)
  void save_to_file(const std::string& path) const;
  void load_weights_file(const std::string& path);
  // BatchNorm running statistics sidecar (path.bnstats, written by save_to_file)
  void load_bn_stats(const std::string& path);
  static Sequential from_file(const std::string& path, Device dev = Device::cpu());

 private:
  std::string name_;
  std::vector<std::unique_ptr<Layer>> layers_;
  std::vector<int64_t> input_chw_;
  Device dev_ = Device::cpu();
  bool training_ = true;
  bool initialized_ = false;
  std::shared_ptr<ParamArena> arena_;
  std::function<void(size_t)> bwd_hook_;
  void pack_params();
};

class SequentialBuilder {
 public:
  explicit SequentialBuilder(std::string name = "sequential") : model_(std::move(name)) {}
  SequentialBuilder& input(const std::vector<int64_t>& chw);
  SequentialBuilder& conv2d(int out_ch, int kh, int kw, int sh = 1, int sw = 1, int ph = 0, int pw = 0,
                            bool bias = true, const std::string& name = "");
  // channels from the running shape
  SequentialBuilder& depthwise_conv2d(int kh, int kw, int sh = 1, int sw = 1, int ph = 0, int pw = 0, bool bias = true,
                                      const std::string& name = "");
  SequentialBuilder& grouped_conv2d(int out_ch, int kh, int kw, int groups, int sh = 1, int sw = 1, int ph = 0,
                                    int pw = 0, bool bias = true, const std::string& name = "");
  SequentialBuilder& batchnorm(float eps = 1e-5f, float momentum = 0.1f, bool affine = true,
                               const std::string& name = "");
  SequentialBuilder& activation(const std::string& kind = "relu", const std::string& name = "");
  SequentialBuilder& maxpool2d(int kh, int kw, int sh = 0, int sw = 0, int ph = 0, int pw = 0,
                               const std::string& name = "");
  SequentialBuilder& avgpool2d(int kh, int kw, int sh = 1, int sw = 1, int ph = 0, int pw = 0,
                               const std::string& name = "");
  SequentialBuilder& flatten(const std::string& name = "");
  SequentialBuilder& dense(int out_features, bool bias = true, const std::string& name = "");
  SequentialBuilder& groupnorm(int num_groups, float eps = 1e-5f, bool affine = true, const std::string& name = "");
  SequentialBuilder& dropout(float rate, const std::string& name = "");
  SequentialBuilder& drop_path(float rate, const std::string& name = "");
  SequentialBuilder& layernorm(float eps = 1e-6f, bool affine = true, const std::string& name = "");
  SequentialBuilder& layer_scale(float init_value = 1e-6f, const std::string& name = "");
  // ConvNeXt block: dw7x7 - LayerNorm - 1x1 (4x) - GELU - 1x1 - LayerScale, identity shortcut, no activation
  // [- DropPath when drop_path > 0, with an explicit seed when has_seed]
  SequentialBuilder& convnext_block(int channels, float layer_scale_init = 1e-6f, const std::string& name = "",
                                    float drop_path = 0.f, bool has_seed = false, uint64_t drop_path_seed = 0);
  // ConvNeXt stage transition: LayerNorm (name_ln), then a 2x2 / stride-2 conv (name_conv)
  SequentialBuilder& convnext_downsample(int out_ch, const std::string& name = "convnext_downsample");
  // generic residual block from prebuilt paths (shapes must agree)
  SequentialBuilder& residual(std::vector<std::unique_ptr<Layer>> main, std::vector<std::unique_ptr<Layer>> shortcut,
                              const std::string& activation = "relu", const std::string& name = "");
  // 3x3-BN-ReLU-3x3-BN (+ 1x1-BN projection when the stride or width changes), ReLU after the add
  // (reference include/nn/sequential.hpp:1253)
  SequentialBuilder& basic_residual_block(int in_ch, int out_ch, int stride = 1, const std::string& name = "");
  // 1x1-BN-ReLU-3x3(stride)-BN-ReLU-1x1-BN, BN eps 1e-3 (reference include/nn/sequential.hpp:1288)
  SequentialBuilder& bottleneck_residual_block(int in_ch, int mid_ch, int out_ch, int stride = 1,
                                               const std::string& name = "");
  SequentialBuilder& resnext_bottleneck_block(int in_ch, int mid_ch, int out_ch, int groups, int stride = 1,
                                              const std::string& name = "");
  Sequential build();

 private:
  std::string auto_name(const std::string& given, const std::string& kind);
  // the conv builders' common ends: the running channel count (input() must have been called),
  // and adding `l` with the running shape moved to its output
  int conv_in() const;
  SequentialBuilder& add_conv(std::unique_ptr<Layer> l);
  Sequential model_;
  std::vector<int64_t> cur_;  // current (C, H, W)
  int count_ = 0;
};

// ---- loss: softmax cross-entropy over logits [N, C] (mean over the batch)
struct LossResult {
  double loss = 0;
  long correct = 0;
  Tensor grad;  // d loss / d logits, same device / dtype as the logits
};
LossResult softmax_cross_entropy(const Tensor& logits, const Tensor& labels);

class Optimizer {
 public:
  explicit Optimizer(float lr) : lr_(lr) {}
  virtual ~Optimizer() = default;
  virtual void step(const std::vector<Param*>& params) = 0;
  void set_learning_rate(float lr) { lr_ = lr; }
  float learning_rate() const { return lr_; }
  // Global-norm gradient clipping (torch's clip_grad_norm_, L2): the step takes g * coef with
  // coef = min(1, max_norm / (norm + 1e-6)) over ALL parameters; the gradient tensors are not
  // rewritten. On a GPU arena the norm stays in device memory (one fixed-order reduction, no host
  // read), so a captured step remains one graph. A non-finite norm propagates; no step is skipped.
  // 0 = off (the default): the step launches what it always launched.
  void set_max_grad_norm(float max_norm);
  float max_grad_norm() const { return max_norm_; }
  // Weight EMA, decay in (0, 1): ema = decay ema + (1 - decay) p_new after each step, a copy of the
  // weights when it is created (prepare(), or the first step). BatchNorm running statistics are
  // not averaged. 0 = off.
  void set_ema_decay(float decay);
  float ema_decay() const { return ema_decay_; }
  // Adam, LAMB and LARS: biases, norm affines and layer scales (Param::no_decay) take the step
  // without weight decay (LAMB and LARS: and with trust 1)
  void set_no_decay_norm_bias(bool on) { no_decay_ = on; }
  bool no_decay_norm_bias() const { return no_decay_; }
  // create what the switches need (EMA buffers, the norm block, the reduction's workspace) now;
  // step() does it on demand, a graph capture needs it done before
  void prepare(const std::vector<Param*>& params);
  // exchange the weights with their EMA (and back with a second call, bit for bit); refreshes the
  // bf16 shadows and the transposed conv operands. Between steps only; no-op with the EMA off.
  void swap_ema(const std::vector<Param*>& params);
  // the gradient norm of the last step before clipping (synchronises the device); NaN with clipping off
  float last_grad_norm() const;
  // What TrainGraph asks of an optimizer whose step it captures: the step reads its scalars (learning
  // rate, step count) from device memory. step_count / set_step_count: the host mirror of the device
  // counter; before_replay: a replay is about to run one step on the device (mirror it, upload a
  // changed learning rate); upload_hyper: host state -> device scalars, outside a capture. The count
  // of an optimizer that does not count its steps (SGD, LARS) stays 0.
  virtual bool capturable() const { return false; }
  virtual long step_count() const { return t_; }
  virtual void set_step_count(long t) { t_ = t; }
  virtual void before_replay();
  virtual void upload_hyper();

 protected:
  bool tail() const { return max_norm_ > 0.f || ema_decay_ > 0.f; }
  // GPU arena: launch the norm reduction, return the device pointer to coef (null with clipping off)
  const float* launch_norm(ParamArena* a);
  // per-parameter path: the coefficient from the norm over all parameters (null with clipping off)
  const double* host_coef(const std::vector<Param*>& params);
  // the EMA buffer of an arena or of a parameter, null with the EMA off
  template <class Owner>
  float* ema_of(Owner* x) const {
    return ema_decay_ > 0.f ? x->ema.template ptr<float>() : nullptr;
  }
  // GPU arena path of a capturable step: create the device scalars, bring them up to date with the
  // host (lr, t), and throw "<what> changed inside a graph capture" if that has to happen in one
  void sync_hyper(ParamArena* a, const char* what);
  float lr_;
  float max_norm_ = 0.f, ema_decay_ = 0.f;
  bool no_decay_ = false;
  long t_ = 0;
  Tensor norm_;                      // device {sumsq, norm, coef, max_norm} (GPU arena path)
  float host_norm_ = std::nanf("");  // per-parameter path
  double host_coef_ = 1.0;
  // step scalars in device memory {lr, bc1, bc2, t} (t and the bias corrections advance on the
  // device) and what the host last uploaded
  Tensor hyper_;
  float hyper_lr_ = -1.f;
  long hyper_t_ = -1;
};

class SGD : public Optimizer {
 public:
  explicit SGD(float lr, float momentum = 0.f) : Optimizer(lr), momentum_(momentum) {}
  void step(const std::vector<Param*>& params) override;
  float momentum() const { return momentum_; }

 private:
  float momentum_;
};

class Adam : public Optimizer {
 public:
  explicit Adam(float lr, float b1 = 0.9f, float b2 = 0.999f, float eps = 1e-8f, float wd = 0.f,
                bool decoupled = false)
      : Optimizer(lr), b1_(b1), b2_(b2), eps_(eps), wd_(wd), decoupled_(decoupled) {}
  void step(const std::vector<Param*>& params) override;
  // (no_decay_norm_bias on the GPU arena path: the arena's block table and a second instance of the
  // fused kernel)
  bool capturable() const override { return true; }
  // a replayed graph runs one step on the device: mirror its count on the host
  void before_replay() override;

 protected:
  float b1_, b2_, eps_, wd_;
  bool decoupled_;
};

// What LAMB and LARS share: a trust ratio per parameter from the L2 norms of its weights and of its
// update, taken on the weights before the step. On a GPU arena the norms are one segmented fixed-order
// reduction over the flat buffers (ParamArena::segments, csrc/kernels/layerwise.hip) and the trust
// table stays on the device: two launches a step, no host read, capturable. With no_decay_norm_bias
// a Param::no_decay parameter takes wd = 0 and trust 1. A zero norm gives trust 1; a non-finite
// norm propagates into that parameter's step.
class LayerwiseState {
 public:
  // the trust ratio of every parameter in the last step (synchronises the device): not for the hot path
  std::vector<float> last_trust_ratios() const;

 protected:
  // GPU arena: the partials and the trust table for `a`'s tables (created outside a capture)
  void workspace(ParamArena* a);
  // per-parameter CPU path: parameter i as one segment of `n` elements
  struct One {
    std::vector<int> chunks, segs;
  };
  static One one_segment(long n, bool adapt);
  // the per-parameter CPU step of `who`: step_one(p, chunks, nchunks, segs, out) makes the cpu_ops
  // call for parameter p as one segment, out[0] becomes its trust ratio
  template <class StepOne>
  void step_each(const std::vector<Param*>& params, const char* who, bool no_decay, StepOne step_one);
  Tensor part_, out_;           // GPU arena path
  size_t nsegs_ = 0;
  std::vector<double> trust_;   // per-parameter path
};

// LAMB (You et al. 2019): Adam's moments, r = (m / bc1) / (sqrt(v / bc2) + eps) + wd p, and
// p -= lr trust r with trust = ||p|| / ||r|| per parameter. State and captured-step protocol as
// Adam's (t, m, v). The betas are kept in double: the kernels take float(1 - beta).
class LAMB : public Adam, public LayerwiseState {
 public:
  explicit LAMB(float lr = 1e-3f, double b1 = 0.9, double b2 = 0.999, float eps = 1e-6f, float wd = 0.01f)
      : Adam(lr, (float)b1, (float)b2, eps, wd, false), b1d_(b1), b2d_(b2) {}
  void step(const std::vector<Param*>& params) override;

 private:
  double b1d_, b2d_;
};

// LARS (You et al. 2017): trust = tc ||p|| / (||g|| + wd ||p|| + eps) per parameter,
// v = mom v - lr trust (g + wd p), p += v (SGD's velocity convention and state; momentum 0: no velocity).
class LARS : public SGD, public LayerwiseState {
 public:
  explicit LARS(float lr = 0.1f, float momentum = 0.9f, float wd = 5e-4f, float trust_coefficient = 1e-3f,
                float eps = 1e-8f)
      : SGD(lr, momentum), wd_(wd), tc_(trust_coefficient), eps_(eps) {}
  void step(const std::vector<Param*>& params) override;
  bool capturable() const override { return true; }

 private:
  float wd_, tc_, eps_;
};


// ---- data
class DataSource {
 public:
  virtual ~DataSource() = default;
  virtual void reset(uint64_t epoch) = 0;
  // next batch: x fp32 host NCHW, labels int64; false at the end of the epoch
  virtual bool next(int batch, Tensor& x, Tensor& labels) = 0;
  virtual size_t size() const = 0;
};

// learnable synthetic classification set: class k images carry a class-specific spatial
// pattern plus noise (deterministic in the seed)
class SyntheticClassification : public DataSource {
 public:
  SyntheticClassification(size_t n, int c, int h, int w, int classes, uint64_t seed, float noise = 0.5f);
  void reset(uint64_t epoch) override;
  bool next(int batch, Tensor& x, Tensor& labels) override;
  size_t size() const override { return n_; }

 private:
  size_t n_;
  int c_, h_, w_, classes_;
  uint64_t seed_;
  float noise_;
  std::vector<float> proto_;
  std::vector<size_t> order_;
  size_t pos_ = 0;
};

struct TrainingConfig {
  int epochs = 1;
  int batch_size = 64;
  int max_steps = -1;          // per epoch, -1 = whole epoch
  int progress_interval = 50;  // steps between progress lines, 0 = quiet
  float lr_decay = 1.0f;       // multiplicative per epoch
  uint64_t seed = 0;
};

struct EpochStats {
  double train_loss = 0, train_acc = 0, val_loss = 0, val_acc = 0, seconds = 0;
};

// one optimisation step; returns (loss, correct)
LossResult train_step(Sequential& model, Optimizer& opt, const Tensor& x, const Tensor& labels);
// mean loss / accuracy over a source
EpochStats evaluate(Sequential& model, DataSource& src, int batch_size);
std::vector<EpochStats> train_classification_model(Sequential& model, DataSource& train, DataSource* val,
                                                   Optimizer& opt, const TrainingConfig& cfg);

}  // namespace dcnn
