"""Argument validation of go1ppo_tail_fwd (include/go1ppo.h): it returns before any launch, so the codes are checked without a GPU, on
made-up addresses that are never dereferenced.  Only calls that must be refused are made.  -1: the table, the number of nets, a net's
input, row count, depth or input leading dimension; -2: a layer's pointers, sizes, chaining or output leading dimension, input rows
narrower than the first layer, an ELU-on-load latent term without its operands; -1 is checked first, over all nets.  (What the
library must ACCEPT - a null out with any ld_out, elu_in without a latent and npv = wz_ld = lat_ld = 0 - is launched by
tests/test_gpu_tail_fwd_fp64.py, where a launch has somewhere to go.)"""
import ctypes

import pytest

BASE = 0x10000          # made-up, 16-byte aligned addresses


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    from go1_gym_learn.ppo_cse import fused
    return fused.load_library(g.build_ppo_hip()), fused


def net(N, k, dims=(512, 256, 128, 64), rows=33, latent=True, **over):
    """fills net k of a table with an acceptable net: three layers behind a 512-wide block of a 1280-wide matrix, ELU on load with a latent"""
    N.in_, N.rows, N.ld_in, N.num_layers = BASE * (100 * k + 1), rows, 1280, len(dims) - 1
    N.elu_in, N.npv, N.lat_ld, N.wz_ld = 1, 2, 64, 64
    N.latent, N.wz = (BASE * (100 * k + 2), BASE * (100 * k + 3)) if latent else (None, None)
    for l in range(len(dims) - 1):
        L = N.layer[l]
        L.W, L.bias, L.out = BASE * (100 * k + 10 + 3 * l), BASE * (100 * k + 11 + 3 * l), BASE * (100 * k + 12 + 3 * l)
        L.n_out, L.k_in, L.ld_out, L.elu = dims[l + 1], dims[l], dims[l + 1], int(l < len(dims) - 2)
    for name, v in over.items():
        setattr(N, name, v)


def table(F, num_nets=2, **over):
    a = F.TailArgs()
    a.num_nets = num_nets
    for k in range(min(max(num_nets, 0), 3)):
        net(a.net[k], k, **over)
    return a


def call(env, a):
    lib, _ = env
    return lib.go1ppo_tail_fwd(ctypes.byref(a), None)


def with_layer(F, l, k=1, **over):
    a = table(F)
    for name, v in over.items():
        setattr(a.net[k].layer[l], name, v)
    return a


def test_minus_one(env):
    lib, F = env
    assert lib.go1ppo_tail_fwd(None, None) == -1
    for n in (0, -1, 4, 100):
        assert call(env, table(F, num_nets=n)) == -1, n
    for over in (dict(in_=None), dict(in_=BASE + 8), dict(in_=BASE + 2), dict(rows=0), dict(rows=-5), dict(num_layers=0), dict(num_layers=-1),
                 dict(num_layers=5), dict(ld_in=1284), dict(ld_in=1281)):
        for k in (0, 1, 2):                                        # in any net of the table
            a = table(F, num_nets=3)
            for name, v in over.items():
                setattr(a.net[k], name, v)
            assert call(env, a) == -1, (over, k)


@pytest.mark.parametrize("l, over", [(0, dict(W=None)), (2, dict(bias=None)), (1, dict(W=BASE + 8)), (0, dict(k_in=0)), (0, dict(k_in=544)),
                                     (0, dict(k_in=496)), (2, dict(n_out=0)), (2, dict(n_out=72)), (2, dict(n_out=528)), (1, dict(n_out=-16)),
                                     (1, dict(k_in=288)), (2, dict(k_in=64)), (1, dict(n_out=96)), (0, dict(ld_out=248)), (2, dict(ld_out=63)),
                                     (2, dict(ld_out=0))])
def test_minus_two_from_a_layer(env, l, over):
    lib, F = env
    for k in (0, 1):
        assert call(env, with_layer(F, l, k, **over)) == -2, k


@pytest.mark.parametrize("over", [dict(ld_in=504), dict(ld_in=8), dict(ld_in=0), dict(wz=None), dict(npv=0), dict(npv=-2), dict(lat_ld=1),
                                  dict(wz_ld=1), dict(npv=5, lat_ld=4, wz_ld=64), dict(npv=5, lat_ld=64, wz_ld=4), dict(lat_ld=0), dict(wz_ld=-64)])
def test_minus_two_from_what_would_leave_the_buffers(env, over):
    """ld_in < layer[0].k_in; elu_in with a latent and a null wz, npv < 1, lat_ld < npv or wz_ld < npv"""
    lib, F = env
    for k in (0, 1, 2):
        a = table(F, num_nets=3)
        for name, v in over.items():
            setattr(a.net[k], name, v)
        assert call(env, a) == -2, k


def test_minus_one_wins_over_minus_two(env):
    lib, F = env
    a = with_layer(F, 0, k=0, W=None)
    assert call(env, a) == -2
    a.net[0].rows = 0
    assert call(env, a) == -1
    a = table(F, ld_in=504)
    assert call(env, a) == -2
    a.net[0].in_ = None
    assert call(env, a) == -1
    a = table(F, wz=None)
    a.net[0].num_layers = 5
    assert call(env, a) == -1
    a = table(F, num_nets=4, wz=None)
    assert call(env, a) == -1
    # a -2 condition in the first net, a -1 condition in the last
    a = table(F, num_nets=3)
    a.net[0].layer[1].n_out = 72
    assert call(env, a) == -2
    a.net[2].ld_in = 1284
    assert call(env, a) == -1
