"""The classifier-head rule of the shared fusion planner (csrc/kernels/fusion_plan.cpp): FF_FUSE_HEAD
on an average pool that is followed by flatten and dense at the end of a sequence, and nowhere
else. CPU: the planner is plain C++."""
import pytest

from dcnn_amd.ops._ext import kernels


@pytest.fixture(scope="module")
def K():
    return kernels()


def test_head_flag_only_on_a_closing_avgpool_flatten_dense(K):
    C, B, R, O = K.FK_CONV, K.FK_BN, K.FK_RELU, K.FK_OTHER
    AP, MP, FL, D = K.FK_AVGPOOL, K.FK_MAXPOOL, K.FK_FLATTEN, K.FK_DENSE
    H = K.FF_FUSE_HEAD
    assert len({C, B, R, K.FK_ACT, O, AP, MP, FL, D}) == 9  # the kinds are distinct
    assert H not in (K.FF_EMIT_BN_STATS, K.FF_FUSE_RELU, K.FF_PASSTHROUGH, K.FF_FUSE_POOL, K.FF_BNB_CONSUMER)
    body = [C, B, R, O, O]
    f = K.plan_sequence_fusions(body + [AP, FL, D])
    assert f[5] == H and f[6] == 0 and f[7] == 0
    assert f[:5] == K.plan_sequence_fusions(body)  # the body's plan is the one without a head
    assert K.plan_sequence_fusions([AP, FL, D]) == [H, 0, 0]
    for kinds in ([AP, FL, D, R],          # something follows the dense layer
                  [AP, FL, D, D],
                  [AP, D],                 # no flatten
                  [C, AP, D],
                  [MP, FL, D],             # a max pool
                  [AP, FL],                # no dense layer
                  [AP, R, FL, D],          # not adjacent
                  [AP, FL, O, D],
                  [FL, D], [D], []):
        assert not any(v & H for v in K.plan_sequence_fusions(kinds)), kinds
    # an earlier pool -> flatten -> dense that does not close the sequence gets nothing; the closing one does
    f = K.plan_sequence_fusions([AP, FL, D, AP, FL, D])
    assert [v & H for v in f] == [0, 0, 0, H, 0, 0]


def test_existing_plans_are_unchanged(K):
    """The cases of tests/test_fusion_plan.py, with and without a head behind them."""
    C, B, R, A, P, O = K.FK_CONV, K.FK_BN, K.FK_RELU, K.FK_ACT, K.FK_MAXPOOL, K.FK_OTHER
    kinds = [C, B, R, P, C, B, R, C, A, B, C, O]
    want = [K.FF_EMIT_BN_STATS, K.FF_FUSE_RELU | K.FF_FUSE_POOL, K.FF_PASSTHROUGH, 0, K.FF_EMIT_BN_STATS,
            K.FF_FUSE_RELU, K.FF_PASSTHROUGH, K.FF_BNB_CONSUMER, 0, 0, K.FF_BNB_CONSUMER, 0]
    assert K.plan_sequence_fusions(kinds) == want
    assert K.plan_sequence_fusions(kinds + [K.FK_AVGPOOL, K.FK_FLATTEN, K.FK_DENSE]) == want + [K.FF_FUSE_HEAD, 0, 0]
    assert K.plan_sequence_fusions([]) == [] and K.plan_sequence_fusions([B]) == [0]
    basic, proj = [C, B, R, C, B], [C, B]
    assert K.plan_residual_fusions(basic, proj, True) == K.RF_FUSED_TAIL | K.RF_DUAL_SHORTCUT
    assert K.plan_residual_fusions(basic, [], True) == K.RF_FUSED_TAIL
    assert K.plan_residual_fusions(basic, proj, False) == 0
