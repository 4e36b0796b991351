"""Argument validation of the rollout entry points of libgo1ppo.so (include/go1ppo.h: go1ppo_act, go1ppo_store_step, go1ppo_gae,
go1ppo_normalize, go1ppo_ring_snapshot, go1ppo_ring_step, go1ppo_ring_gather): it returns before any launch, so the codes are checked
without a GPU, on made-up addresses that are never dereferenced.  Only calls that must be refused are made; every one returns -1."""
import pytest

BASE = 0x10000          # made-up, 16-byte aligned addresses

ACT = ("mean", "value", "head_ld", "std", "num_actions", "rows", "noise", "actions", "mu", "sigma", "values", "logp")
STORE = ("rewards", "dones", "time_outs", "env_bins", "values", "gamma", "n", "rewards_out", "dones_out", "env_bins_out")
GAE = ("rewards", "dones", "values", "last_values", "T", "N", "gamma", "lam", "returns", "advantages", "stats")
NORM = ("adv", "n", "stats")
SNAPSHOT = ("hist", "ld_hist", "N", "H", "no", "ring")
STEP = ("obs", "priv", "ring_dst", "ring_window", "N", "H", "no", "npv", "Kp", "X", "obs_store", "priv_store")
GATHER = ("ring", "priv_store", "idx", "rows", "N", "H", "no", "npv", "Kp", "X")
SCALARS = dict(head_ld=64, num_actions=12, rows=320, gamma=0.99, lam=0.95, n=320, T=7, N=320, ld_hist=2100, H=30, no=70, npv=2, Kp=2104)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from go1_gym_learn.ppo_cse import fused
    return fused.load_library(g.build_ppo_hip())


def call(lib, fn, names, **over):
    """the entry point on an acceptable argument set with `over` laid on top: pointers are distinct made-up addresses"""
    v = {k: SCALARS.get(k, BASE * (i + 1)) for i, k in enumerate(names)}
    assert set(over) <= set(names), over
    v.update(over)
    return getattr(lib, fn)(*[v[k] for k in names], None)


def refused(lib, fn, names, null, ranges):
    for field in null:
        assert call(lib, fn, names, **{field: None}) == -1, (fn, field)
    for over in ranges:
        assert call(lib, fn, names, **over) == -1, (fn, over)


def test_act(lib):
    refused(lib, "go1ppo_act", ACT, ("mean", "value", "std", "noise", "actions", "mu", "sigma", "values", "logp"),
            (dict(rows=0), dict(rows=-3), dict(num_actions=0), dict(num_actions=-1), dict(num_actions=65), dict(num_actions=12, head_ld=11),
             dict(num_actions=1, head_ld=0)))


def test_store_step(lib):
    refused(lib, "go1ppo_store_step", STORE, ("rewards", "dones", "values", "rewards_out", "dones_out"),
            (dict(n=0), dict(n=-1), dict(env_bins_out=None), dict(env_bins_out=None, time_outs=None)))
    # the optional inputs absent: a required pointer alone decides
    for field in ("rewards", "dones", "values", "rewards_out", "dones_out"):
        assert call(lib, "go1ppo_store_step", STORE, time_outs=None, env_bins=None, env_bins_out=None, **{field: None}) == -1, field


def test_gae(lib):
    refused(lib, "go1ppo_gae", GAE, ("rewards", "dones", "values", "last_values", "returns", "advantages", "stats"),
            (dict(T=0), dict(T=-1), dict(N=0), dict(N=-5), dict(N=4096 * 256 + 1), dict(N=1 << 40)))


def test_normalize(lib):
    refused(lib, "go1ppo_normalize", NORM, ("adv", "stats"), (dict(n=0), dict(n=-1)))


def test_ring_snapshot(lib):
    refused(lib, "go1ppo_ring_snapshot", SNAPSHOT, ("hist", "ring"),
            (dict(N=0), dict(N=-1), dict(H=0), dict(H=-1), dict(no=0), dict(no=-2), dict(no=69), dict(ld_hist=2099), dict(ld_hist=0)))


def test_ring_step(lib):
    refused(lib, "go1ppo_ring_step", STEP, ("obs", "priv", "ring_window", "X"),
            (dict(N=0), dict(N=-1), dict(H=0), dict(H=-1), dict(no=0), dict(no=-2), dict(no=69), dict(npv=-1), dict(npv=257, Kp=2400),
             dict(Kp=2105), dict(Kp=2102), dict(Kp=2100), dict(npv=4, Kp=2104)))
    # with the optional pointers absent as well
    for field in ("obs", "priv", "ring_window", "X"):
        assert call(lib, "go1ppo_ring_step", STEP, ring_dst=None, obs_store=None, priv_store=None, **{field: None}) == -1, field


def test_ring_gather(lib):
    refused(lib, "go1ppo_ring_gather", GATHER, ("ring", "priv_store", "idx", "X"),
            (dict(rows=0), dict(rows=-1), dict(N=0), dict(N=-1), dict(H=0), dict(H=-1), dict(no=0), dict(no=-2), dict(no=69), dict(npv=-1),
             dict(Kp=2105), dict(Kp=2102), dict(Kp=2100), dict(npv=4, Kp=2104)))
