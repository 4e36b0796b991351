"""Argument validation of go1ppo_mlp2_tail_ppo / go1ppo_mlp2_tail_mse (include/go1ppo.h): it returns before any launch, so the codes are
checked without a GPU, on made-up addresses that are never dereferenced.  -1: a null pointer, a row count or a loss parameter out of
range; -2: a leading dimension, an alignment or a buffer that does not match between the nets and the loss; -1 is checked first."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    from go1_gym_learn.ppo_cse import fused
    return fused.load_library(g.build_ppo_hip()), fused


BASE = 0x10000          # made-up, 16-byte aligned addresses


def tail(F, k, rows=320, **over):
    a = F.Mlp2Tail()
    for i, name in enumerate(("x", "W2", "b2", "W3", "b3", "z2", "out", "d_out", "d_z2", "d_x")):
        setattr(a, name, BASE * (16 * k + i + 1))
    a.rows, a.ld_x, a.ld_z2, a.ld_out, a.ld_dout, a.ld_dz2, a.ld_dx, a.elu_input = rows, 256, 128, 64, 64, 128, 256, 1
    for name, v in over.items():
        setattr(a, name, v)
    return a


def loss(F, nets, **over):
    a = F.LossArgs()
    for i, name in enumerate(("std", "idx", "actions", "old_mu", "old_sigma", "old_logp", "advantages", "returns", "old_values", "d_std",
                              "d_mean_bias", "d_value_bias", "kl", "value_loss", "surrogate_loss")):
        setattr(a, name, BASE * (64 + i))
    a.mean, a.value, a.d_mean, a.d_value = nets[0].out, nets[1].out, nets[0].d_out, nets[1].d_out
    a.head_ld, a.num_actions, a.rows, a.clip_param, a.use_clipped_value_loss = 64, 12, nets[0].rows, 0.2, 1
    for name, v in over.items():
        setattr(a, name, v)
    return a


def call_ppo(env, nets, la):
    lib, F = env
    arr = (F.Mlp2Tail * 2)(*nets)
    return lib.go1ppo_mlp2_tail_ppo(arr, ctypes.byref(la), None)


def mse(F, net, **over):
    q = F.MseArgs()
    q.target, q.idx, q.d_pred_bias, q.train_loss, q.test_loss = BASE * 80, BASE * 81, BASE * 82, BASE * 83, BASE * 84
    q.num_train, q.npv, q.selective = net.rows // 5 * 4, 2, 0
    for name, v in over.items():
        setattr(q, name, v)
    return q


def call_mse(env, net, q):
    lib, F = env
    return lib.go1ppo_mlp2_tail_mse(ctypes.byref(net), ctypes.byref(q), None)


def test_ppo_tail_null_and_range(env):
    lib, F = env
    nets = [tail(F, 0), tail(F, 1)]
    assert lib.go1ppo_mlp2_tail_ppo(None, ctypes.byref(loss(F, nets)), None) == -1
    assert lib.go1ppo_mlp2_tail_ppo((F.Mlp2Tail * 2)(*nets), None, None) == -1
    for field in ("x", "W2", "b2", "W3", "b3", "z2", "out", "d_out", "d_z2", "d_x"):
        for k in (0, 1):
            bad = [tail(F, 0), tail(F, 1)]
            setattr(bad[k], field, None)
            assert call_ppo(env, bad, loss(F, nets)) == -1, (field, k)
    for field in ("std", "idx", "actions", "old_mu", "old_sigma", "old_logp", "advantages", "returns", "old_values"):
        assert call_ppo(env, nets, loss(F, nets, **{field: None})) == -1, field
    assert call_ppo(env, [tail(F, 0, rows=0), tail(F, 1, rows=0)], loss(F, nets, rows=0)) == -1
    for A in (0, -1, 13, 16, 33):
        assert call_ppo(env, nets, loss(F, nets, num_actions=A)) == -1, A
    # the old values are not read without the clipped value loss: their pointer may be null then (-2 here: the next check that fails)
    assert call_ppo(env, nets, loss(F, nets, old_values=None, use_clipped_value_loss=0, head_ld=72)) == -2


@pytest.mark.parametrize("over", [dict(ld_x=260), dict(ld_x=248), dict(ld_z2=132), dict(ld_z2=120), dict(ld_out=72), dict(ld_dout=128),
                                  dict(ld_dz2=124), dict(ld_dx=250), dict(x=BASE + 8), dict(W2=BASE * 2 + 2), dict(W3=BASE * 4 + 4),
                                  dict(b2=BASE * 3 + 4), dict(b3=BASE * 5 + 2), dict(z2=BASE * 6 + 8), dict(out=BASE * 7 + 8),
                                  dict(d_out=BASE * 8 + 8), dict(d_z2=BASE * 9 + 8), dict(d_x=BASE * 10 + 4),
                                  dict(d_z2=BASE * 6), dict(d_x=BASE)])
def test_tails_bad_shape_or_alignment(env, over):
    """-2 from either entry point; the last two: d_z2 on z2, d_x on x"""
    lib, F = env
    good = [tail(F, 0), tail(F, 1)]
    for k in (0, 1):
        nets = [tail(F, 0), tail(F, 1)]
        nets[k] = tail(F, k, **{n: (v + BASE * 16 * k if n[0] != "l" else v) for n, v in over.items()})
        assert call_ppo(env, nets, loss(F, nets)) == -2, k
    assert call_mse(env, tail(F, 0, **over), mse(F, good[0])) == -2


def test_ppo_tail_loss_must_match_the_nets(env):
    lib, F = env
    nets = [tail(F, 0), tail(F, 1)]
    for over in (dict(head_ld=72), dict(rows=319), dict(mean=BASE * 99), dict(value=BASE * 99), dict(d_mean=BASE * 99), dict(d_value=BASE * 99)):
        assert call_ppo(env, nets, loss(F, nets, **over)) == -2, over
    assert call_ppo(env, [tail(F, 0), tail(F, 1, rows=256)], loss(F, nets)) == -2


def test_mse_tail_null_and_range(env):
    lib, F = env
    net = tail(F, 0)
    assert lib.go1ppo_mlp2_tail_mse(None, ctypes.byref(mse(F, net)), None) == -1
    assert lib.go1ppo_mlp2_tail_mse(ctypes.byref(net), None, None) == -1
    for field in ("x", "W2", "b2", "W3", "b3", "z2", "out", "d_out", "d_z2", "d_x"):
        assert call_mse(env, tail(F, 0, **{field: None}), mse(F, net)) == -1, field
    for field in ("target", "idx", "train_loss", "test_loss"):
        assert call_mse(env, net, mse(F, net, **{field: None})) == -1, field
    for over in (dict(num_train=0), dict(num_train=320), dict(num_train=-3), dict(npv=0), dict(npv=65)):
        assert call_mse(env, net, mse(F, net, **over)) == -1, over
    assert call_mse(env, tail(F, 0, rows=0), mse(F, net)) == -1


def test_minus_one_wins_over_minus_two(env):
    lib, F = env
    nets = [tail(F, 0, ld_x=260), tail(F, 1, z2=BASE * 22 + 2)]
    assert call_ppo(env, nets, loss(F, nets)) == -2
    assert call_ppo(env, nets, loss(F, nets, num_actions=16)) == -1
    assert call_ppo(env, nets, loss(F, nets, idx=None)) == -1
    nets[1].W3 = None
    assert call_ppo(env, nets, loss(F, nets)) == -1
    bad = tail(F, 0, ld_dout=72)
    assert call_mse(env, bad, mse(F, bad)) == -2
    assert call_mse(env, bad, mse(F, bad, num_train=320)) == -1
    assert call_mse(env, bad, mse(F, bad, target=None)) == -1
