// Cross-language parity probe of the C++ host API (tests/test_cpp_host_blocks.py drives it):
//
//   host_api_parity schedulers                 LR sequence of every scheduler type, one line each
//   host_api_parity losses <in.bin> <C>        loss + gradient of the six losses on a [N, C] record
//                                              (labels = row index % C), CPU backend
//   host_api_parity forward <model> <x.bin> [--device GPU]
//                                              logits of a saved model (path.json/.bin/.bnstats) in
//                                              eval mode for an (N, C, H, W) .bin record
//   host_api_parity grads <model_name> <batch> <out.bin> [<prefix>] [--device GPU]
//                                              one forward + backward; every parameter gradient
//                                              (logical NCHW fp32 records) into out.bin; with a
//                                              prefix also the initial model (prefix.json/.bin)
//                                              and the batch (prefix.x.bin, prefix.y.bin)
//   host_api_parity blocks <model_name> <batch> [--device GPU]
//                                              teacher-forced per-layer errors against the CPU backend
//   host_api_parity resblock <in> <out> <hw> <batch> <out.bin> [--device GPU]
//                                              one stride-2 basic residual block, forward + backward on
//                                              fixed data; its input gradient and parameter gradients
//   host_api_parity train <model_name> <steps> <batch> <save> [--device GPU] [--graph] [--adamw-no-decay]
//                         [--mix] [--switch-to-labels] [--clip-ema MAX_NORM] [--opt lamb|lars]
//                                              Adam steps on a synthetic set, then save
//                                              (--opt lamb|lars: LAMB / LARS steps instead, the trust
//                                              ratios of the last step printed; dumps as --clip-ema)
//                                              (--clip-ema: global-norm clipping at MAX_NORM and a
//                                              weight EMA of decay 0.9; the EMA weights are saved
//                                              too, as <save>.ema, and the last gradient norm printed;
//                                              the initial model goes to <save>.init and batch i to
//                                              <save>.x<i>.bin / <save>.y<i>.bin; with --graph every
//                                              step runs through TrainGraph, on the CPU as well)
//   grads / train also take [--drop-path RATE] [--seed-drop-path] (ConvNeXt models)
// Output is plain text: one "key v0 v1 ..." line per item.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>

#include "dcnn/nn.hpp"
#include "dcnn/train.hpp"

using namespace dcnn;

// --drop-path RATE: the ConvNeXt models' stochastic depth; --seed-drop-path: block k's DropPath gets
// the explicit seed 1000 + k (a checkpoint then draws the same masks in the Python front end)
static float drop_path_arg(int argc, char** argv) {
  for (int i = 1; i + 1 < argc; ++i)
    if (std::string(argv[i]) == "--drop-path") return (float)std::atof(argv[i + 1]);
  return 0.f;
}
static bool flag_arg(int argc, char** argv, const char* f) {
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == f) return true;
  return false;
}
// "convnext_two_block" (not a zoo model): 3x16x16 input, 2x2 / stride-2 stem to 16 channels, two
// ConvNeXt blocks (layer scale 0.5) with DropPath at rate 0.5 and explicit seeds, pool, LayerNorm, fc
static const char* kTwoBlock = "convnext_two_block";
static int input_hw(const std::string& name) {
  return name == kTwoBlock ? 16 : name.find("cifar") != std::string::npos ? 32 : 64;
}
static int num_classes(const std::string& name) {
  return name == kTwoBlock || name.find("cifar") != std::string::npos ? 10 : 200;
}
static Sequential model_arg(int argc, char** argv, const std::string& name) {
  if (name == kTwoBlock) {
    SequentialBuilder b("cnx_dp");
    b.input({3, 16, 16}).conv2d(16, 2, 2, 2, 2, 0, 0, true, "stem_conv").layernorm(1e-6f, true, "stem_ln")
        .convnext_block(16, 0.5f, "block1", 0.5f, true, 101)
        .convnext_block(16, 0.5f, "block2", 0.5f, true, (1ull << 40) + 7);
    return b.avgpool2d(8, 8, 1, 1, 0, 0, "avgpool").layernorm(1e-6f, true, "head_ln").flatten("flatten")
        .dense(10, true, "fc").build();
  }
  return create_model(name, drop_path_arg(argc, argv), flag_arg(argc, argv, "--seed-drop-path") ? 1000 : 0);
}

static Device device_arg(int argc, char** argv) {
  for (int i = 1; i + 1 < argc; ++i)
    if (std::string(argv[i]) == "--device") return Device::parse(argv[i + 1]);
  return Device::cpu();
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: host_api_parity schedulers|losses|forward|train ...\n");
    return 2;
  }
  const std::string cmd = argv[1];
  try {
    if (cmd == "schedulers") {
      const char* cfgs[] = {
          R"({"type": "step_lr", "parameters": {"step_size": 3, "gamma": 0.5}})",
          R"({"type": "multi_step_lr", "parameters": {"milestones": [2, 5, 9], "gamma": 0.3}})",
          R"({"type": "exponential_lr", "parameters": {"gamma": 0.9}})",
          R"({"type": "cosine_annealing_lr", "parameters": {"T_max": 7, "eta_min": 0.001}})",
          R"({"type": "cosine_annealing_warm_restarts", "parameters": {"T_0": 3, "T_mult": 2, "eta_min": 0.0}})",
          R"({"type": "linear_warmup", "parameters": {"warmup_steps": 4, "start_lr": 0.01}})",
          R"({"type": "warmup_cosine_annealing", "parameters": {"warmup_steps": 3, "total_steps": 10, "start_lr": 0.0, "eta_min": 0.01}})",
          R"({"type": "reduce_lr_on_plateau", "parameters": {"mode": "min", "factor": 0.5, "patience": 2, "threshold": 0.0001, "min_lr": 0.001}})",
          R"({"type": "polynomial_lr", "parameters": {"total_steps": 8, "power": 2.0, "end_lr": 0.001}})",
          R"({"type": "one_cycle_lr", "parameters": {"max_lr": 0.5, "total_steps": 10, "pct_start": 0.3, "div_factor": 25.0, "final_div_factor": 10000.0}})",
      };
      for (const char* c : cfgs) {
        SGD opt(0.1f);
        auto s = SchedulerFactory::create_from_config(json::Value::parse(c), &opt);
        std::printf("%s %.9g", s->type().c_str(), (double)opt.learning_rate());
        const double metrics[] = {1.0, 0.9, 0.95, 0.95, 0.96, 0.97, 0.5, 0.6, 0.6, 0.6, 0.7, 0.8};
        for (int k = 0; k < 12; ++k) {
          if (s->type() == "reduce_lr_on_plateau")
            s->step(metrics[k]);
          else
            s->step();
          std::printf(" %.9g", (double)opt.learning_rate());
        }
        std::printf("\n");
      }
      return 0;
    }
    if (cmd == "losses" && argc >= 4) {
      std::ifstream f(argv[2], std::ios::binary);
      Tensor x = Tensor::load(f);
      const int C = std::atoi(argv[3]);
      const int N = (int)(x.numel() / C);
      Tensor pred = x.view({N, C});
      std::vector<int64_t> lab(N);
      for (int i = 0; i < N; ++i) lab[i] = i % C;
      Tensor labels = Tensor::from_host_i64(lab, Device::cpu());
      const char* names[] = {"crossentropy", "softmax_crossentropy", "logsoftmax_crossentropy", "mse", "mae", "huber"};
      for (const char* n : names) {
        Loss l = LossFactory::create(n);
        LossResult r = l.compute(pred, &labels);
        std::printf("%s %.9g %ld", n, r.loss, r.correct);
        for (float g : r.grad.to_host_f32()) std::printf(" %.9g", (double)g);
        std::printf("\n");
      }
      return 0;
    }
    if (cmd == "forward" && argc >= 4) {
      const Device dev = device_arg(argc, argv);
      Sequential m = Sequential::from_file(argv[2], dev);
      m.set_training(false);
      std::ifstream f(argv[3], std::ios::binary);
      Tensor x = Tensor::load(f);
      Tensor logits = m.forward(x);
      std::printf("params %zu\nlogits", m.num_parameters());
      for (float v : logits.to_host_f32()) std::printf(" %.9g", (double)v);
      std::printf("\n");
      return 0;
    }
    if (cmd == "grads" && argc >= 5) {
      // one forward + backward on the first synthetic batch; every parameter's gradient is
      // written (logical NCHW fp32 records, parameter order) to argv[4]
      const Device dev = device_arg(argc, argv);
      Sequential m = model_arg(argc, argv, argv[2]);
      m.set_device(dev);
      m.initialize(11);
      const int batch = std::atoi(argv[3]);
      const int hw = input_hw(argv[2]), classes = num_classes(argv[2]);
      SyntheticClassification data((size_t)batch, 3, hw, hw, classes, 5, 0.3f);
      // --mix: every batch through a BatchMixer (Mixup 0.8 / CutMix 1.0, seed 7), trained against its
      // dense target with soft_crossentropy (label smoothing 0.1); --switch-to-labels: the last step
      // is fed the integer labels instead (a captured step must refuse them)
      const bool mix = flag_arg(argc, argv, "--mix"), sw = flag_arg(argc, argv, "--switch-to-labels");
      BatchMixer mixer(classes, 0.8, 1.0, 1.0, 0.5, 7);
      Loss loss = mix ? LossFactory::create("soft_crossentropy", 0.1f) : LossFactory::create("softmax_crossentropy");
      data.reset(0);
      Tensor x, y;
      if (!data.next(batch, x, y)) throw std::runtime_error("no batch");
      if (argc >= 6 && argv[5][0] != '-') {
        // the initial weights and the batch, for another front end to run the same step
        const std::string pre = argv[5];
        m.save_to_file(pre);
        std::ofstream fx(pre + ".x.bin", std::ios::binary);
        x.to(Device::cpu()).save(fx);
        std::vector<float> yl;
        for (int64_t v : y.to(Device::cpu()).to_host_i64()) yl.push_back((float)v);
        std::ofstream fy(pre + ".y.bin", std::ios::binary);
        Tensor::from_host(yl, {(int64_t)yl.size(), 1, 1, 1}, Device::cpu()).save(fy);
      }
      m.zero_grad();
      LossResult r = loss(m.forward(x), y);
      m.backward(r.grad);
      std::ofstream f(argv[4], std::ios::binary);
      std::printf("loss %.9g\nparams", r.loss);
      for (Param* p : m.parameters()) {
        p->grad.view(p->shape, p->layout).save(f);
        std::printf(" %s", p->name.c_str());
      }
      std::printf("\n");
      return 0;
    }
    if (cmd == "resblock" && argc >= 7) {
      // one basic downsample residual block (stride 2, projection shortcut) alone: forward and
      // backward on fixed pseudo-random data; the input gradient, then every parameter gradient
      const Device dev = device_arg(argc, argv);
      const int in = std::atoi(argv[2]), out = std::atoi(argv[3]), hw = std::atoi(argv[4]), batch = std::atoi(argv[5]);
      Sequential m = SequentialBuilder("downsample_block").input({in, hw, hw}).basic_residual_block(in, out, 2, "block").build();
      m.set_device(dev);
      m.initialize(11);
      m.set_training(true);
      uint32_t lcg = 12345u;
      auto fill = [&](size_t n) {
        std::vector<float> v(n);
        for (float& f : v) {
          lcg = lcg * 1664525u + 1013904223u;
          f = ((float)(lcg >> 8) / (float)(1u << 24) - 0.5f) * 2.f;
        }
        return v;
      };
      auto act = [&](const std::vector<float>& v, const std::vector<int64_t>& shape) {
        return Tensor::from_host(v, shape, dev, dev.is_gpu() ? DType::BF16 : DType::F32,
                                 dev.is_gpu() ? Layout::NHWC : Layout::NCHW);
      };
      Layer* block = m.layers()[0].get();
      block->set_input_grad(true);
      m.zero_grad();
      const Tensor x = act(fill((size_t)batch * in * hw * hw), {batch, in, hw, hw});
      const Tensor y = block->forward(x, true);
      const Tensor dx = block->backward(act(fill((size_t)y.numel()), y.shape()));
      std::ofstream f(argv[6], std::ios::binary);
      Tensor::from_host(dx.to_host_f32(), dx.shape(), Device::cpu()).save(f);
      std::printf("params dx");
      for (Param* p : m.parameters()) {
        p->grad.view(p->shape, p->layout).save(f);
        std::printf(" %s", p->name.c_str());
      }
      std::printf("\n");
      return 0;
    }
    if (cmd == "blocks" && argc >= 4) {
      // teacher-forced per segment (a top-level layer, or a BatchNorm with the activation / pool
      // the GPU backend fuses into it): the CPU backend's fp32 activations and gradients of one
      // step are the reference; every GPU segment gets the CPU input and output gradient, and its
      // output, input gradient and parameter gradients are compared. Errors do not compound
      // through the network, so each layer's bound is absolute (tests/test_cpp_host_blocks.py).
      const std::string name = argv[2];
      const int batch = std::atoi(argv[3]);
      const Device gdev = device_arg(argc, argv);
      Sequential mc = create_model(name), mg = create_model(name);
      mc.set_device(Device::cpu());
      mc.initialize(11);
      mg.set_device(gdev);
      mg.initialize(11);
      mc.set_training(true);
      mg.set_training(true);
      const bool cifar = name.find("cifar") != std::string::npos;
      const int hw = cifar ? 32 : 64, classes = cifar ? 10 : 200;
      SyntheticClassification data((size_t)batch, 3, hw, hw, classes, 5, 0.3f);
      data.reset(0);
      Tensor x, y;
      if (!data.next(batch, x, y)) throw std::runtime_error("no batch");
      const auto& lc = mc.layers();
      const auto& lg = mg.layers();
      const size_t L = lc.size();
      // CPU reference: every top-level activation and gradient
      mc.zero_grad();
      std::vector<Tensor> act(L + 1), grad(L + 1);
      act[0] = mc.input_activation(x);
      for (size_t i = 0; i < L; ++i) act[i + 1] = lc[i]->forward(act[i], true);
      const Tensor logits = act[L].view({act[L].dim(0), act[L].numel() / act[L].dim(0)});
      Loss loss = LossFactory::create("softmax_crossentropy");
      LossResult r = loss(logits, y);
      grad[L] = r.grad.view(act[L].shape(), Layout::NCHW);
      lc[0]->set_input_grad(false);
      for (size_t i = L; i-- > 0;) grad[i] = lc[i]->backward(grad[i + 1]);
      auto cosine = [](const std::vector<float>& a, const std::vector<float>& b) {
        double ab = 0, aa = 0, bb = 0;
        for (size_t k = 0; k < a.size() && k < b.size(); ++k) {
          ab += (double)a[k] * b[k];
          aa += (double)a[k] * a[k];
          bb += (double)b[k] * b[k];
        }
        return aa > 0 && bb > 0 ? ab / std::sqrt(aa * bb) : (aa == bb ? 1.0 : 0.0);
      };
      auto rel = [](const std::vector<float>& a, const std::vector<float>& b) {
        double num = 0, den = 0;
        for (size_t k = 0; k < a.size() && k < b.size(); ++k) {
          num += ((double)a[k] - b[k]) * ((double)a[k] - b[k]);
          den += (double)b[k] * b[k];
        }
        return a.size() != b.size() ? 1e9 : std::sqrt(num / (den > 1e-300 ? den : 1e-300));
      };
      // GPU activation of a CPU tensor (bf16 NHWC for 4-D activations)
      auto to_gpu = [&](const Tensor& t) {
        return Tensor::from_host(t.to_host_f32(), t.shape(), gdev, gdev.is_gpu() ? DType::BF16 : DType::F32,
                                 gdev.is_gpu() ? Layout::NHWC : Layout::NCHW);
      };
      mg.zero_grad();
      lg[0]->set_input_grad(false);
      for (size_t i = 0; i < L;) {
        size_t j = i + 1;
        if (auto* bn = dynamic_cast<BatchNorm*>(lg[i].get())) {
          if (gdev.is_gpu() && bn->fused_relu() && j < L) ++j;  // (its ReLU runs in the BatchNorm)
          if (gdev.is_gpu() && bn->fused_pool() && j < L) ++j;  // (and the max-pool)
        }
        Tensor h = i == 0 ? mg.input_activation(x) : to_gpu(act[i]);
        for (size_t k = i; k < j; ++k) h = lg[k]->forward(h, true);
        const double ef = rel(h.to_host_f32(), act[j].to_host_f32());
        Tensor g = to_gpu(grad[j]);
        for (size_t k = j; k-- > i;) g = lg[k]->backward(g);
        double eb = 0, cb = 1;
        if (i > 0 && g.defined()) {
          // (a conv whose input a BatchNorm + ReLU produced returns its data gradient already
          // masked by that ReLU — the mask runs in the dgrad epilogue with the BatchNorm's backward
          // statistics — so the reference is the CPU gradient masked by input > 0 there; the
          // closer of the two references is reported)
          const auto gg = g.to_host_f32(), gc = grad[i].to_host_f32(), xin = act[i].to_host_f32();
          std::vector<float> gm(gc.size());
          for (size_t k = 0; k < gc.size(); ++k) gm[k] = xin[k] > 0.f ? gc[k] : 0.f;
          const double e0 = rel(gg, gc), e1 = rel(gg, gm);
          eb = std::min(e0, e1);
          cb = e1 < e0 ? cosine(gg, gm) : cosine(gg, gc);
        }
        // parameter gradients: error relative to max(|ref|, 5% of the segment's largest gradient)
        // (a conv bias in front of a BatchNorm has a mathematically zero gradient: noise on both)
        double ep = 0, cp = 1;
        std::string pn;
        std::vector<std::pair<std::vector<float>, std::vector<float>>> pairs;
        std::vector<std::string> names;
        double scale = 0;
        for (size_t k = i; k < j; ++k) {
          std::vector<Param*> pc, pg;
          lc[k]->collect_params(pc);
          lg[k]->collect_params(pg);
          for (size_t q = 0; q < pc.size() && q < pg.size(); ++q) {
            pairs.emplace_back(pg[q]->grad.view(pg[q]->shape, pg[q]->layout).to_host_f32(),
                               pc[q]->grad.view(pc[q]->shape, pc[q]->layout).to_host_f32());
            names.push_back(pg[q]->name);
            double nb = 0;
            for (float v : pairs.back().second) nb += (double)v * v;
            scale = std::max(scale, std::sqrt(nb));
          }
        }
        for (size_t q = 0; q < pairs.size(); ++q) {
          const auto& [a, b] = pairs[q];
          double num = 0, nb = 0;
          for (size_t k = 0; k < a.size(); ++k) {
            num += ((double)a[k] - b[k]) * ((double)a[k] - b[k]);
            nb += (double)b[k] * b[k];
          }
          const double e = std::sqrt(num) / std::max(std::sqrt(nb), 0.05 * scale + 1e-30);
          if (e > ep) {
            ep = e;
            pn = names[q];
          }
          if (std::sqrt(nb) >= 0.05 * scale) cp = std::min(cp, cosine(a, b));
        }
        std::printf("segment %zu %zu %s fwd %.6g bwd %.6g param %.6g %s bcos %.6g pcos %.6g\n", i, j,
                    lg[i]->name().c_str(), ef, eb, ep, pn.empty() ? "-" : pn.c_str(), cb, cp);
        i = j;
      }
      return 0;
    }
    if (cmd == "train" && argc >= 6) {
      const Device dev = device_arg(argc, argv);
      Sequential m = model_arg(argc, argv, argv[2]);
      m.set_device(dev);
      m.initialize(11);
      const int steps = std::atoi(argv[3]), batch = std::atoi(argv[4]);
      const int hw = input_hw(argv[2]), classes = num_classes(argv[2]);
      SyntheticClassification data((size_t)batch * steps, 3, hw, hw, classes, 5, 0.3f);
      // --adamw-no-decay: AdamW, weight decay 0.1, biases / norm affines / layer scales excluded
      const bool nd = flag_arg(argc, argv, "--adamw-no-decay");
      // --opt lamb|lars: the layer-wise optimizers, biases / norm affines / layer scales excluded
      // (LAMB lr 1e-3, weight decay 0.1; LARS lr 0.5, momentum 0.9, weight decay 0.01, tc 0.02)
      std::string oname;
      float clip = 0.f;
      for (int i = 1; i + 1 < argc; ++i) {
        if (std::string(argv[i]) == "--clip-ema") clip = (float)std::atof(argv[i + 1]);
        if (std::string(argv[i]) == "--opt") oname = argv[i + 1];
      }
      std::unique_ptr<Optimizer> optp;
      LayerwiseState* lw = nullptr;
      if (oname == "lamb") {
        auto o = std::make_unique<LAMB>(1e-3f, 0.9, 0.999, 1e-6f, 0.1f);
        o->set_no_decay_norm_bias(true);
        lw = o.get();
        optp = std::move(o);
      } else if (oname == "lars") {
        auto o = std::make_unique<LARS>(0.5f, 0.9f, 0.01f, 0.02f, 1e-8f);
        o->set_no_decay_norm_bias(true);
        lw = o.get();
        optp = std::move(o);
      } else if (oname.empty() || oname == "adam") {
        auto o = std::make_unique<Adam>(1e-3f, 0.9f, 0.999f, 1e-8f, nd ? 0.1f : 0.f, nd);
        o->set_no_decay_norm_bias(nd);
        optp = std::move(o);
      } else {
        throw std::invalid_argument("--opt " + oname + ": adam, lamb or lars");
      }
      Optimizer& opt = *optp;
      const bool dump = clip > 0.f || lw != nullptr;  // the initial model and every batch, for a replay elsewhere
      if (clip > 0.f) {
        opt.set_max_grad_norm(clip);
        opt.set_ema_decay(0.9f);
      }
      // --mix: every batch through a BatchMixer (Mixup 0.8 / CutMix 1.0, seed 7), trained against its
      // dense target with soft_crossentropy (label smoothing 0.1); --switch-to-labels: the last step
      // is fed the integer labels instead (a captured step must refuse them)
      const bool mix = flag_arg(argc, argv, "--mix"), sw = flag_arg(argc, argv, "--switch-to-labels");
      BatchMixer mixer(classes, 0.8, 1.0, 1.0, 0.5, 7);
      Loss loss = mix ? LossFactory::create("soft_crossentropy", 0.1f) : LossFactory::create("softmax_crossentropy");
      data.reset(0);
      Tensor x, y;
      bool graph = false;  // --graph: the GPU step captured once (TrainGraph) and replayed
      for (int i = 1; i < argc; ++i) graph = graph || std::string(argv[i]) == "--graph";
      TrainGraph tg(m, opt, loss);
      if (dump) m.save_to_file(std::string(argv[5]) + ".init");
      std::printf("losses");
      for (int i = 0; i < steps && data.next(batch, x, y); ++i) {
        if (dump) {
          const std::string pre = std::string(argv[5]) + ".";
          std::ofstream fx(pre + "x" + std::to_string(i) + ".bin", std::ios::binary);
          x.to(Device::cpu()).save(fx);
          std::vector<float> yl;
          for (int64_t v : y.to(Device::cpu()).to_host_i64()) yl.push_back((float)v);
          std::ofstream fy(pre + "y" + std::to_string(i) + ".bin", std::ios::binary);
          Tensor::from_host(yl, {(int64_t)yl.size(), 1, 1, 1}, Device::cpu()).save(fy);
        }
        if (mix && !(sw && i == steps - 1)) {
          Tensor xd = x.to(dev).clone(), t;
          mixer.mix(xd, y, t);
          x = xd;
          y = t;
        }
        if (graph && (dev.is_gpu() || dump)) {
          const double l = tg.step(x, y);
          std::printf(" %.6g", dev.is_gpu() ? tg.last_loss() : l);
          continue;
        }
        m.zero_grad();
        LossResult r = loss(m.forward(x), y);
        m.backward(r.grad);
        opt.step(m.parameters());
        std::printf(" %.6g", r.loss);
      }
      std::printf("\n");
      m.save_to_file(argv[5]);
      if (lw != nullptr) {
        std::printf("trust");
        for (float t : lw->last_trust_ratios()) std::printf(" %.9g", (double)t);
        std::printf("\n");
      }
      if (clip > 0.f) {
        std::printf("grad_norm %.9g\n", (double)opt.last_grad_norm());
        opt.swap_ema(m.parameters());
        m.save_to_file(std::string(argv[5]) + ".ema");
        opt.swap_ema(m.parameters());
      }
      return 0;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "bad arguments\n");
  return 2;
}
