"""The rollout half of libgo1ppo.so (csrc/go1ppo.hip: go1ppo_act, go1ppo_store_step, go1ppo_gae, go1ppo_normalize, go1ppo_ring_snapshot /
_step / _gather) against the float64 and integer models of tests/ppo_rollout_ref.py, over the tables of cases that module holds, and
once each through the Python side (fused.act, fused.store_step, RolloutStorage._compute_returns_fused, fused.ring_step, fused.ring_gather).

Buffer discipline as in test_gpu_ppo_loss_fp64.py: every buffer sits inside canaries (7), the canaries are checked after the launch,
inputs are compared with their copies, and every case is launched twice on fresh copies of its outputs: the two results are bit for bit
the same.  The bounds are derived in ppo_rollout_ref.py, none is taken from what the kernels give; what that module calls bit for bit is
held against a zero bound.  Each test prints its largest error-to-bound ratios (run with -s); profiles/ppo_rollout_fp64.txt keeps the
figures measured on an MI355X.  Every launch is one the library accepts: indices in range, buffers of full length."""
import numpy as np
import pytest
import torch

import ppo_rollout_ref as R
from test_gpu_ppo_loss_fp64 import RATIOS, Mat, Vec, note, worst
from test_gpu_ppo_tail_fused import PAD, stream

pytestmark = pytest.mark.gpu

FAMILIES = ("rollout act", "rollout store_step", "rollout gae", "rollout normalize", "rollout ring", "rollout wrappers")


@pytest.fixture(scope="module")
def lib():
    from go1_gym_learn.ppo_cse import fused
    yield fused.load_library()
    for fam in FAMILIES:
        if fam in RATIOS:
            print(f"\nppo_rollout_fp64 family [{fam}]: " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(RATIOS[fam].items())), end="")
    print()


def t(a):
    """numpy -> CPU tensor of the same bits (bf16 bit patterns travel as int16)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def bf(bits):
    return t(bits).view(torch.bfloat16)


def host(x):
    a = x.contiguous().cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def filled(n, dtype=torch.float32):
    """an output of n elements that starts as canary values"""
    return Vec(torch.full((n,), 7, dtype=dtype))


def addr(v, elements=0):
    """address of element `elements` of a Vec (of an empty one too: its place between the canaries)"""
    return v.flat.data_ptr() + (PAD + v.off + elements) * v.flat.element_size()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def run_twice(inputs, outputs, launch):
    """launch(out) -> return code, on fresh copies `out` of the outputs, twice; what the first launch left behind"""
    results = []
    for _ in (0, 1):
        out = {k: b.clone() for k, b in outputs.items()}
        before = {k: b.flat.clone() for k, b in inputs.items()}
        rc = launch(out)
        torch.cuda.synchronize()
        assert rc == 0
        for k, b in inputs.items():
            assert same_bits(b.flat, before[k]), f"input {k} was written"
        for k, b in out.items():
            assert b.canaries_intact(), f"{k}: a canary was written"
        results.append(out)
    for k in outputs:
        assert same_bits(results[0][k].flat, results[1][k].flat), f"launch 1: {k} differs from launch 0"
    return results[0]


def ratios_of(checks):
    """{name: (err, bound)} -> {name: worst ratio}, asserting every bound; the ring's per-step rows count as one figure"""
    out = {}
    for k, (e, b) in checks.items():
        r = worst(torch.from_numpy(np.ascontiguousarray(e, np.float64)).flatten(), torch.from_numpy(np.ascontiguousarray(b, np.float64)).flatten())
        k = "X" if k[0] == "X" and k[1:].isdigit() else k
        out[k] = max(out.get(k, 0.0), r)
    return out


def first_nonzero(codes):
    return next((rc for rc in codes if rc != 0), 0)


# ------------------------------------------------------------------------------------------------------------------ go1ppo_act
@pytest.mark.parametrize("c", R.ACT_CASES, ids=lambda c: c.name)
def test_act_kernel_matches_the_fp64_model(lib, c):
    d = R.act_inputs(c)
    rows, A = c.rows, c.A
    head = Mat(rows, c.head_ld, bf(d["head"]))
    inputs = dict(head=head, std=Vec(t(d["std"])), noise=Vec(t(d["noise"])))
    if c.shared:
        value_ptr = head.ptr() + A * 2                             # column A of the buffer that holds mean
    else:
        inputs["value_head"] = Mat(rows, c.head_ld, bf(d["value_head"]))
        value_ptr = inputs["value_head"].ptr()
    outputs = dict(actions=filled(rows * A), mu=filled(rows * A), sigma=filled(rows * A), values=filled(rows), logp=filled(rows))

    def launch(o):
        return lib.go1ppo_act(head.ptr(), value_ptr, c.head_ld, addr(inputs["std"]), A, rows, addr(inputs["noise"]), addr(o["actions"]), addr(o["mu"]),
                              addr(o["sigma"]), addr(o["values"]), addr(o["logp"]), stream())
    out = run_twice(inputs, outputs, launch)
    got = {k: host(out[k].v).reshape(rows, A) for k in ("actions", "mu", "sigma")}
    got.update({k: host(out[k].v) for k in ("values", "logp")})
    note("rollout act", c.name, **ratios_of(R.act_compare(d, got)))


# ------------------------------------------------------------------------------------------------------------------ go1ppo_store_step
@pytest.mark.parametrize("c", R.STORE_CASES, ids=lambda c: c.name)
def test_store_step_kernel_matches_the_fp64_model(lib, c):
    d = R.store_inputs(c)
    inputs = {k: Vec(t(d[k])) for k in ("rewards", "dones", "values", "time_outs", "env_bins") if d[k] is not None}
    outputs = dict(rewards_out=filled(c.n), dones_out=filled(c.n, torch.uint8), env_bins_out=filled(c.n))
    opt = lambda k: addr(inputs[k]) if k in inputs else None

    def launch(o):
        # env_bins_out is given even where env_bins is not: it must then keep what it holds
        return lib.go1ppo_store_step(addr(inputs["rewards"]), addr(inputs["dones"]), opt("time_outs"), opt("env_bins"), addr(inputs["values"]), d["gamma"],
                                     c.n, addr(o["rewards_out"]), addr(o["dones_out"]), addr(o["env_bins_out"]), stream())
    out = run_twice(inputs, outputs, launch)
    note("rollout store_step", c.name, **ratios_of(R.store_compare(d, {k: host(b.v) for k, b in out.items()})))


# ------------------------------------------------------------------------------------------------------------------ go1ppo_gae
def gae_buffers(d):
    return {k: Vec(t(d[k])) for k in ("rewards", "dones", "values", "last_values")}


def gae_launch(lib, d, inputs, o):
    c = d["case"]
    return lib.go1ppo_gae(addr(inputs["rewards"]), addr(inputs["dones"]), addr(inputs["values"]), addr(inputs["last_values"]), c.T, c.N, d["gamma"],
                          d["lam"], addr(o["returns"]), addr(o["advantages"]), addr(o["stats"]), stream())


@pytest.mark.parametrize("c", R.GAE_CASES, ids=lambda c: c.name)
def test_gae_kernel_matches_the_fp64_model(lib, c):
    d = R.gae_inputs(c)
    inputs = gae_buffers(d)
    start = R.gae_stats_start(d)
    outputs = dict(returns=filled(c.T * c.N), advantages=filled(c.T * c.N), stats=Vec(t(start)))
    out = run_twice(inputs, outputs, lambda o: gae_launch(lib, d, inputs, o))
    got = {k: host(out[k].v).reshape(c.T, c.N) for k in ("returns", "advantages")}
    checks = R.gae_compare(d, got)
    checks["stats"] = R.gae_stats_check(got["advantages"], start, host(out["stats"].v), c.T, c.N)
    note("rollout gae", c.name, **ratios_of(checks))


def test_gae_ticket_counter_over_changing_grids(lib):
    """launches of 1, 2, 4, 1 and 5 workgroups and back, onto stats that nobody zeroes in between: a ticket counter that one launch
    left unequal to 0 lets a later, smaller launch publish nothing (or an early arriver publish a part)"""
    T = 3
    order = R.TICKET_N + R.TICKET_N[::-1]
    cases = [R.gae_inputs(R.GaeCase(f"ticket-{i}-N{N}", T, N, "random", 1.0, R.GAMMA, R.LAM)) for i, N in enumerate(order)]
    finals = []
    for _ in (0, 1):
        stats = Vec(t(np.zeros(2)))
        ref, bound, worst_ratio = np.zeros(2), np.zeros(2), {}
        for d in cases:
            c = d["case"]
            inputs = gae_buffers(d)
            o = dict(returns=filled(T * c.N), advantages=filled(T * c.N), stats=stats)
            assert gae_launch(lib, d, inputs, o) == 0
            torch.cuda.synchronize()
            assert all(b.canaries_intact() for b in o.values())
            got = {k: host(o[k].v).reshape(T, c.N) for k in ("returns", "advantages")}
            checks = R.gae_compare(d, got)
            # this launch's additions on top of what the earlier ones may have lost
            err, b = R.gae_stats_check(got["advantages"], ref, host(stats.v), T, c.N)
            sums, _ = R.gae_stat_terms(got["advantages"])
            ref, bound = ref + sums, bound + b
            checks["stats"] = (np.abs(host(stats.v) - ref), bound)
            for k, v in ratios_of(checks).items():
                worst_ratio[k] = max(worst_ratio.get(k, 0.0), v)
        finals.append(stats)
    assert same_bits(finals[0].flat, finals[1].flat)
    note("rollout gae", "ticket counter, ten launches", **worst_ratio)


# ------------------------------------------------------------------------------------------------------------------ go1ppo_normalize
@pytest.mark.parametrize("c", R.NORM_CASES, ids=lambda c: c.name)
def test_normalize_kernel_matches_the_fp64_model(lib, c):
    d = R.norm_inputs(c)
    inputs = dict(stats=Vec(t(d["stats"])))
    out = run_twice(inputs, dict(adv=Vec(t(d["adv"]))), lambda o: lib.go1ppo_normalize(addr(o["adv"]), c.n, addr(inputs["stats"]), stream()))
    got = host(out["adv"].v)
    assert np.isfinite(got).all()
    note("rollout normalize", c.name, **ratios_of(R.norm_compare(d, got)))


# ------------------------------------------------------------------------------------------------------------------ observation ring
def ring_direct(lib, d):
    """a rollout of T steps through the library: snapshot from a history view with ld_hist > H * no, ring_step with a null ring_dst at
    s = 0 and row s + H - 1 of the same ring from then on, the last step once more with null obs_store / priv_store, and a gather of
    ring_gather_idx (descending, duplicates, entries of the last step)"""
    c = d["case"]
    N, T, H, no, npv, Kp = c.N, c.T, c.H, c.no, c.npv, c.Kp
    idx = R.ring_gather_idx(c)
    assert idx.min() >= 0 and idx.max() < T * N and d["ld_hist"] > H * no
    inputs = dict(hist=Vec(t(d["hist"])), idx=Vec(t(idx)))
    for s in range(T):
        inputs[f"obs{s}"], inputs[f"priv{s}"] = Vec(t(d["stream"][s + H - 1])), Vec(t(d["priv"][s]))
    i16 = torch.int16
    outputs = dict(ring=filled((T + H - 1) * N * no, i16), gathered=filled(idx.size * Kp, i16), X_null=filled(N * Kp, i16),
                   obs_store=filled(T * N * no), priv_store=filled(T * N * npv))
    outputs.update({f"X{s}": filled(N * Kp, i16) for s in range(T)})

    def launch(o):
        row = lambda r: addr(o["ring"], r * N * no)
        codes = [lib.go1ppo_ring_snapshot(addr(inputs["hist"]), d["ld_hist"], N, H, no, row(0), stream())]
        for s in range(T):
            dst = None if s == 0 else row(s + H - 1)
            codes.append(lib.go1ppo_ring_step(addr(inputs[f"obs{s}"]), addr(inputs[f"priv{s}"]), dst, row(s), N, H, no, npv, Kp, addr(o[f"X{s}"]),
                                              addr(o["obs_store"], s * N * no), addr(o["priv_store"], s * N * npv), stream()))
        codes.append(lib.go1ppo_ring_step(addr(inputs[f"obs{T - 1}"]), addr(inputs[f"priv{T - 1}"]), dst, row(T - 1), N, H, no, npv, Kp, addr(o["X_null"]),
                                          None, None, stream()))
        codes.append(lib.go1ppo_ring_gather(row(0), addr(o["priv_store"]), addr(inputs["idx"]), idx.size, N, H, no, npv, Kp, addr(o["gathered"]), stream()))
        return first_nonzero(codes)
    out = run_twice(inputs, outputs, launch)
    got = dict(ring=host(out["ring"].v).reshape(T + H - 1, N, no), gathered=host(out["gathered"].v).reshape(idx.size, Kp),
               X=[host(out[f"X{s}"].v).reshape(N, Kp) for s in range(T)], obs_store=host(out["obs_store"].v).reshape(T, N, no),
               priv_store=host(out["priv_store"].v).reshape(T, N, npv))
    checks = R.ring_compare(d, got)
    checks["X_null_stores"] = R.bit_diff(host(out["X_null"].v), host(out[f"X{T - 1}"].v))
    return ratios_of(checks)


@pytest.mark.parametrize("c", R.RING_CASES, ids=lambda c: c.name)
def test_ring_kernels_match_the_integer_model(lib, c):
    note("rollout ring", c.name, **ring_direct(lib, R.ring_inputs(c)))


def test_ring_conversion_on_the_rounding_patterns(lib):
    """observations and privileged observations that are ties, just beside a tie, the largest finite numbers (to infinity), +-0,
    +-inf, the smallest normal and NaNs: bf16 round to nearest even bit for bit, a NaN stays a NaN, the fp32 copies keep every bit"""
    d = R.ring_inputs(R.RING_PATTERN_CASE, patterns=True)
    assert set(R.rounding_patterns().tolist()) <= set(d["stream"].view(np.uint32).ravel().tolist())
    note("rollout ring", R.RING_PATTERN_CASE.name, **ring_direct(lib, d))


def test_ring_through_the_storage_wrappers(lib):
    from go1_gym_learn.ppo_cse import fused
    from go1_gym_learn.ppo_cse.rollout_storage import RolloutStorage
    c = R.RING_WRAPPER_CASE
    d = R.ring_inputs(c)
    N, T, H, no, npv = c.N, c.T, c.H, c.no, c.npv
    idx = R.ring_gather_idx(c)
    results = []
    for _ in (0, 1):
        st = RolloutStorage(N, T, [no], [npv], [H * no], [12], "cuda:0", history_dtype=torch.bfloat16, history_pad_to=8, augment=True, ring=True)
        assert st.padded_width == c.Kp and st.history_length == H
        st.obs_ring.view(torch.int16).fill_(7)
        hist = t(d["hist"]).cuda()[:, :H * no]                     # a view: its row stride is ld_hist
        X = [torch.full((N, c.Kp), 7.0, dtype=torch.bfloat16, device="cuda") for _ in range(T)]
        for s in range(T):
            fused.ring_step(lib, st, s, t(d["stream"][s + H - 1]).cuda(), t(d["priv"][s]).cuda(), hist if s == 0 else None, X[s])
        G = torch.full((idx.size, c.Kp), 7.0, dtype=torch.bfloat16, device="cuda")
        fused.ring_gather(lib, st, t(idx).cuda(), G)
        torch.cuda.synchronize()
        results.append(dict(ring=host(st.obs_ring.view(torch.int16)), gathered=host(G.view(torch.int16)), X=[host(x.view(torch.int16)) for x in X],
                            obs_store=host(st.observations), priv_store=host(st.privileged_observations)))
    first, second = results
    for k in ("ring", "gathered", "obs_store", "priv_store"):
        assert R.passes(dict(x=R.bit_diff(first[k], second[k]))), k
    assert all(R.passes(dict(x=R.bit_diff(a, b))) for a, b in zip(first["X"], second["X"]))
    note("rollout ring", c.name, **ratios_of(R.ring_compare(d, first)))


# ------------------------------------------------------------------------------------------------------------------ through the wrappers
def test_act_store_step_and_returns_through_the_wrappers(lib):
    """fused.act (its _ld and pointers, value as a column of mean's buffer), fused.store_step (its optional pointers) and
    RolloutStorage._compute_returns_fused (the stats buffer zeroed per call, stats[2] = T * N) over a rollout of T steps"""
    from go1_gym_learn.ppo_cse import fused
    from go1_gym_learn.ppo_cse.rollout_storage import RolloutStorage
    N, T, A = 257, 3, 12
    st = RolloutStorage(N, T, [4], [2], [8], [A], "cuda:0")
    worst_ratio = {}

    def keep(prefix, checks):
        for k, v in ratios_of(checks).items():
            worst_ratio[f"{prefix}.{k}"] = max(worst_ratio.get(f"{prefix}.{k}", 0.0), v)
    for s in range(T):
        da = R.act_inputs(R.ActCase(f"wrapper-act-{s}", N, A, 64, True))
        heads = bf(da["head"]).cuda()
        fused.act(lib, heads[:, :A], heads[:, A:A + 1], t(da["std"]).cuda(), t(da["noise"]).cuda(), st, s)
        torch.cuda.synchronize()
        keep("act", R.act_compare(da, dict(actions=host(st.actions[s]), mu=host(st.mu[s]), sigma=host(st.sigma[s]), values=host(st.values[s]).ravel(),
                                           logp=host(st.actions_log_prob[s]).ravel())))
        ds = R.store_inputs(R.StoreCase(f"wrapper-store-{s}", N, s != 1, s != 2, 0.05))       # step 1 without time-outs, step 2 without bins
        ds["values"] = host(st.values[s]).ravel()
        ds["dones"] = (ds["dones"] < 26).astype(np.uint8)           # flags, as the scan below reads them
        st.env_bins[s].fill_(7.0)
        opt = lambda k: None if ds[k] is None else t(ds[k]).cuda()
        fused.store_step(lib, st, s, t(ds["rewards"]).cuda(), t(ds["dones"]).cuda(), opt("time_outs"), opt("env_bins"), R.GAMMA)
        torch.cuda.synchronize()
        keep("store_step", R.store_compare(ds, dict(rewards_out=host(st.rewards[s]).ravel(), dones_out=host(st.dones[s]).ravel(),
                                                    env_bins_out=host(st.env_bins[s]).ravel())))
    dg = dict(case=R.GaeCase("wrapper-gae", T, N, "random", 1.0, R.GAMMA, R.LAM), rewards=host(st.rewards).reshape(T, N), values=host(st.values).reshape(T, N),
              dones=host(st.dones).reshape(T, N), last_values=R.gae_inputs(R.GaeCase("wrapper-last", 1, N, "none", 1.0, R.GAMMA, R.LAM))["last_values"],
              gamma=R.GAMMA, lam=R.LAM)
    assert 0 < dg["dones"].sum() < T * N
    # the un-normalised advantages, which the storage does not keep: one direct launch on buffers of its own
    inputs = gae_buffers(dg)
    o = dict(returns=filled(T * N), advantages=filled(T * N), stats=Vec(t(np.zeros(2))))
    assert gae_launch(lib, dg, inputs, o) == 0
    torch.cuda.synchronize()
    adv = host(o["advantages"].v).reshape(T, N)
    runs = []
    for _ in (0, 1):
        st.compute_returns(t(dg["last_values"]).cuda().view(N, 1), R.GAMMA, R.LAM, fused_lib=lib)
        torch.cuda.synchronize()
        runs.append((st.returns.clone(), st.advantages.clone(), st._gae_stats.clone()))
    assert all(same_bits(a, b) for a, b in zip(*runs)), "the second call differs from the first: the stats were not zeroed?"
    stats = host(st._gae_stats)
    assert stats[2] == float(T * N)
    assert same_bits(st.returns.view(T, N), o["returns"].v.view(T, N))
    checks = dict(returns=R.gae_compare(dg, dict(returns=host(st.returns).reshape(T, N), advantages=adv))["returns"],
                  stats=R.gae_stats_check(adv, np.zeros(2), stats[:2], T, N))
    nd = dict(case=R.NormCase("wrapper-normalize", T * N, "plain", 0.0, 1.0), adv=adv.ravel(), stats=stats)
    checks["advantages"] = R.norm_compare(nd, host(st.advantages).ravel())["advantages"]
    keep("returns", checks)
    note("rollout wrappers", "act, store_step, compute_returns", **worst_ratio)
