// The shared fusion planner (fusion_plan.cpp): the cross-layer fusions of a layer sequence on the
// GPU path, one rule set for both front ends (the Python layers and the C++ host API). Plain C++
// (no HIP types), so host-only translation units include it too.
#pragma once
#include <vector>

namespace dcnn {

// layer kinds in order -> per-layer FF_* flags
enum FuseKind : int {
  FK_OTHER = 0, FK_CONV = 1, FK_BN = 2, FK_RELU = 3, FK_ACT = 4, FK_MAXPOOL = 5, FK_AVGPOOL = 6, FK_FLATTEN = 7,
  FK_DENSE = 8, FK_LSCALE = 9, FK_DROPPATH = 10
};
enum FuseFlag : int {
  FF_EMIT_BN_STATS = 1,  // conv: its epilogue emits the statistics rows of the BatchNorm after it
  FF_FUSE_RELU = 2,      // BatchNorm: its apply pass applies the ReLU after it
  FF_PASSTHROUGH = 4,    // ReLU: already applied by the BatchNorm before it
  FF_FUSE_POOL = 8,      // BatchNorm: its training apply also runs the max-pool two layers on
  FF_BNB_CONSUMER = 16,  // conv: its data gradient carries the backward of the BatchNorm [+ ReLU] before it
  // average pool: the sequence ends average pool -> flatten -> dense, the classifier head; the
  // pool's forward also runs the dense layer and the dense layer's backward also the pool's
  // (head.hip, where the geometry allows; flatten passes through)
  FF_FUSE_HEAD = 32,
};
std::vector<int> plan_sequence_fusions(const std::vector<int>& kinds);
// residual block (main path kinds, shortcut kinds, block activation relu / linear / none):
// RF_FUSED_TAIL = the main path's closing BatchNorm applies the shortcut sum and the activation;
// RF_DUAL_SHORTCUT = the shortcut's closing BatchNorm shares that pass;
// RF_SCALE_TAIL = the main path closes in a LayerScale, the shortcut is the identity and the block
// has no activation (act_identity: none / linear): the LayerScale's store adds the block input,
// and the first layer's data gradient adds the shortcut gradient (no separate add either way);
// RF_DROP_TAIL (always with RF_SCALE_TAIL) = the main path closes in LayerScale, DropPath under the
// same conditions: that store also applies the DropPath's per-sample mask (lscale_drop_fwd / _bwd).
// A DropPath anywhere else is FK_OTHER to every rule: the block takes the plain path.
enum ResidualFlag : int { RF_FUSED_TAIL = 1, RF_DUAL_SHORTCUT = 2, RF_SCALE_TAIL = 4, RF_DROP_TAIL = 8 };
int plan_residual_fusions(const std::vector<int>& main_kinds, const std::vector<int>& short_kinds, bool act_ok,
                          bool act_identity = false);

}  // namespace dcnn
