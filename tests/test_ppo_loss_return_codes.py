"""Argument validation of go1ppo_loss / go1ppo_mse (include/go1ppo.h): it returns before any launch, so the codes are checked without a
GPU, on made-up addresses that are never dereferenced.  Only calls that must be refused are made.  -1: a null required pointer, a row
count, an action count or a leading dimension out of range; the six sums of the loss and d_pred_bias are optional, and old_values is
required exactly when the clipped value loss reads it."""
import ctypes

import pytest

BASE = 0x10000          # made-up, 16-byte aligned addresses
LOSS_REQUIRED = ("mean", "value", "std", "idx", "actions", "old_mu", "old_sigma", "old_logp", "advantages", "returns", "d_mean", "d_value")
LOSS_OPTIONAL = ("d_std", "d_mean_bias", "d_value_bias", "kl", "value_loss", "surrogate_loss")
MSE_ARGS = ("pred", "pred_ld", "target", "npv", "idx", "rows", "num_train", "selective", "d_pred", "d_pred_bias", "train_loss", "test_loss")
MSE_REQUIRED = ("pred", "target", "idx", "d_pred", "train_loss", "test_loss")


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    from go1_gym_learn.ppo_cse import fused
    return fused.load_library(g.build_ppo_hip()), fused


def loss(F, **over):
    a = F.LossArgs()
    for i, name in enumerate(LOSS_REQUIRED + ("old_values",) + LOSS_OPTIONAL):
        setattr(a, name, BASE * (i + 1))
    a.head_ld, a.num_actions, a.rows, a.clip_param, a.use_clipped_value_loss = 64, 12, 320, 0.2, 1
    for name, v in over.items():
        setattr(a, name, v)
    return a


def call_loss(env, **over):
    lib, F = env
    return lib.go1ppo_loss(ctypes.byref(loss(F, **over)), None)


def call_mse(env, **over):
    lib, _ = env
    v = dict(pred=BASE, pred_ld=64, target=BASE * 2, npv=2, idx=BASE * 3, rows=320, num_train=256, selective=0, d_pred=BASE * 4,
             d_pred_bias=BASE * 5, train_loss=BASE * 6, test_loss=BASE * 7)
    v.update(over)
    return lib.go1ppo_mse(*[v[k] for k in MSE_ARGS], None)


def test_loss_null_pointers(env):
    lib, F = env
    assert lib.go1ppo_loss(None, None) == -1
    for field in LOSS_REQUIRED:
        assert call_loss(env, **{field: None}) == -1, field
        # whatever else is absent: a required pointer alone decides
        assert call_loss(env, **{field: None}, **{k: None for k in LOSS_OPTIONAL}) == -1, field


def test_loss_old_values_are_required_exactly_when_clipped(env):
    assert call_loss(env, old_values=None, use_clipped_value_loss=1) == -1
    assert call_loss(env, old_values=None, use_clipped_value_loss=7) == -1
    # without the clipped value loss a null old_values is not what refuses a call: the code is that of the other defect alone
    # (no call that would be accepted is made here: there is no GPU to run it)
    assert call_loss(env, old_values=None, use_clipped_value_loss=0, rows=0) == -1
    assert call_loss(env, old_values=None, use_clipped_value_loss=0, mean=None) == -1


def test_loss_ranges(env):
    for over in (dict(rows=0), dict(rows=-5), dict(rows=(1 << 20) + 1), dict(num_actions=0), dict(num_actions=-1), dict(num_actions=33),
                 dict(head_ld=11), dict(head_ld=0), dict(num_actions=32, head_ld=31)):
        assert call_loss(env, **over) == -1, over


def test_mse_null_pointers(env):
    for field in MSE_REQUIRED:
        assert call_mse(env, **{field: None}) == -1, field
        assert call_mse(env, **{field: None}, d_pred_bias=None) == -1, field


def test_mse_ranges(env):
    for over in (dict(rows=0), dict(rows=-1), dict(rows=(1 << 20) + 1, num_train=5), dict(num_train=0), dict(num_train=-2), dict(num_train=320),
                 dict(num_train=400), dict(npv=0), dict(npv=-1), dict(npv=65, pred_ld=72), dict(npv=9, pred_ld=8)):
        assert call_mse(env, **over) == -1, over
