"""The fixed-order cross-workgroup sums of the PPO update (det_last, csrc/go1ppo.hip) through their four entry points at production
shapes: go1ppo_loss and go1ppo_mse (24576-row mini-batch, 12 actions), go1ppo_gae (4096 environments x 24 steps) and
go1ppo_wgrad_tn_batched (the problem table of the fused PPO backward pass, planned by go1ppo_wgrad_tn_plan).

The slab rows are published without a release fence (write-through stores, drained, then a relaxed ticket) and the last arriver reads
them behind one acquire.  A last arriver that read a stale copy of the slab — say, its own L1 lines from the previous launch of the
site — or a counter left unreset would show here:
  * inputs A, then B, then B again: the two B results are bit-equal and match a float64 reference (tolerances of
    tests/test_gpu_ppo_fused.py);
  * a launch with another row count (another grid, another number of contributors) in between, then B once more: bit-equal to B;
  * one captured graph of 20 launches alternating A and B, replayed: every launch's result bit-equal to its eager one."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

M, NA, R = 24576, 12, 98304                      # mini-batch rows, actions, storage rows (4096 envs x 24 steps)
ENVS, STEPS = 4096, 24


@pytest.fixture(scope="module")
def lib():
    from go1_gym_learn.ppo_cse import fused
    return fused.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def check_publication(make):
    """make(seed, size) -> (launch, result, check, keep): launch() sets the destinations and launches on the current stream, result() a
    copy of the destinations, check(r) compares r with the float64 reference; keep holds every buffer the launch reads or writes"""
    A, B, C = make(1, "full"), make(2, "full"), make(3, "other")
    A[0]()
    B[0]()
    b1 = B[1]()
    B[0]()
    b2 = B[1]()
    torch.cuda.synchronize()
    assert torch.equal(b1, b2), (b1 - b2).abs().max()
    B[2](b1)
    A[0]()
    a = A[1]()
    torch.cuda.synchronize()
    A[2](a)
    assert not torch.equal(a, b1)                                 # two different inputs: a stale read would be visible
    C[0]()
    c = C[1]()
    B[0]()
    b3 = B[1]()
    torch.cuda.synchronize()
    C[2](c)
    assert torch.equal(b3, b1), (b3 - b1).abs().max()
    graph, recs = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(graph):
        for i in range(20):
            X = A if i % 2 == 0 else B
            X[0]()
            recs.append(X[1]())
    graph.replay()
    torch.cuda.synchronize()
    for i, r in enumerate(recs):
        assert torch.equal(r, a if i % 2 == 0 else b1), (i, (r - (a if i % 2 == 0 else b1)).abs().max())


def close(got, ref, rtol, atol, what):
    err = (got.double() - ref).abs()
    bound = atol + rtol * ref.abs()
    assert bool((err <= bound).all()), (what, float((err - bound).max()), got, ref)


# ---------------------------------------------------------------------------------------------- loss
def loss_case(lib, seed, size):
    from go1_gym_learn.ppo_cse import fused
    from go1_gym_learn.ppo_cse.ppo import PPO_Args as P
    rows = M if size == "full" else 10000
    g = gen(10 + seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    st = dict(actions=rnd(R, NA), mu=rnd(R, NA) * 0.3, sigma=torch.rand(R, NA, device="cuda", generator=g) + 0.5, logp=rnd(R) * 0.5 - 14.0,
              adv=rnd(R), returns=rnd(R), values=rnd(R))
    idx = torch.randperm(R, device="cuda", generator=g)[:rows]
    mean_b = torch.zeros(rows, 64, device="cuda", dtype=torch.bfloat16)
    mean_b[:, :NA] = (st["mu"][idx] + 0.05 * rnd(rows, NA)).to(torch.bfloat16)
    value_b = torch.zeros(rows, 64, device="cuda", dtype=torch.bfloat16)
    value_b[:, :1] = (st["values"][idx] + 0.3 * rnd(rows)).to(torch.bfloat16).unsqueeze(1)
    std = torch.rand(NA, device="cuda", generator=g) + 0.6
    HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
    mu, sd = mean_b[:, :NA].double(), std.double()
    z = (st["actions"][idx].double() - mu) / sd
    logp = (-0.5 * z * z - torch.log(sd) - HALF_LOG_2PI).sum(-1)
    st["logp"][idx] = (logp + 0.15 * rnd(rows).double()).float()     # ratios straddle the clip range
    dmean = torch.zeros(rows, 64, device="cuda", dtype=torch.bfloat16)
    dvalue = torch.zeros(rows, 64, device="cuda", dtype=torch.bfloat16)
    out = torch.zeros(4 + 2 * NA, device="cuda")                  # sur, vl, kl, dvb, dstd[NA], dmb[NA]
    a = fused.LossArgs()
    a.mean, a.value, a.std, a.head_ld, a.num_actions, a.rows = mean_b.data_ptr(), value_b.data_ptr(), std.data_ptr(), 64, NA, rows
    a.idx = idx.data_ptr()
    a.actions, a.old_mu, a.old_sigma = st["actions"].data_ptr(), st["mu"].data_ptr(), st["sigma"].data_ptr()
    a.old_logp, a.advantages, a.returns, a.old_values = (st[k].data_ptr() for k in ("logp", "adv", "returns", "values"))
    a.clip_param, a.value_loss_coef, a.entropy_coef, a.use_clipped_value_loss = P.clip_param, P.value_loss_coef, P.entropy_coef, 1
    a.d_mean, a.d_value = dmean.data_ptr(), dvalue.data_ptr()
    a.surrogate_loss, a.value_loss, a.kl, a.d_value_bias = (out[i:].data_ptr() for i in range(4))
    a.d_std, a.d_mean_bias = out[4:].data_ptr(), out[4 + NA:].data_ptr()

    def launch():
        out.zero_()
        assert lib.go1ppo_loss(ctypes.byref(a), stream()) == 0

    def check(r):
        b = {k: v[idx].double() for k, v in st.items()}
        ratio = torch.exp(logp - b["logp"])
        lo, hi = 1.0 - P.clip_param, 1.0 + P.clip_param
        s1, s2 = -b["adv"] * ratio, -b["adv"] * ratio.clamp(lo, hi)
        sur_t = torch.maximum(s1, s2) / rows
        v, vo, ret = value_b[:, 0].double(), b["values"], b["returns"]
        vc = vo + (v - vo).clamp(-P.clip_param, P.clip_param)
        vl_t = torch.maximum((v - ret) ** 2, (vc - ret) ** 2) / rows
        so, mo = b["sigma"], b["mu"]
        kl_t = (torch.log(sd / so + 1e-5) + (so * so + (mo - mu) ** 2) / (2.0 * sd * sd) - 0.5).sum(-1) / rows
        for i, t in enumerate((sur_t, vl_t, kl_t)):                # fp32 sums of `rows` terms: relative to the sum, floored by the terms' scale
            close(r[i], t.sum(), 2e-4, 2e-6 * float(t.abs().sum()), ("loss", i))
        inside = (ratio >= lo) & (ratio <= hi)
        dlogp = torch.where(inside | (s1 > s2), -b["adv"], torch.zeros_like(ratio)) * ratio / rows
        per = dlogp[:, None] * (z * z - 1.0) / sd
        # a sample whose ratio sits on a clip edge may take the other branch in fp32: its share is added to the bound
        edge = ((ratio - lo).abs() < 1e-5) | ((ratio - hi).abs() < 1e-5)
        slack = (b["adv"].abs() * ratio / rows)[:, None] * ((z * z - 1.0).abs() / sd)
        close(r[4:4 + NA], per.sum(0) - P.entropy_coef / sd, 2e-3, 2e-5 + slack[edge].sum(0), "d_std")
        close(r[4 + NA:], dmean[:, :NA].double().sum(0), 1e-3, 1e-6, "d_mean_bias")
        close(r[3], dvalue[:, 0].double().sum(), 1e-3, 1e-6, "d_value_bias")

    return launch, lambda: out.clone(), check, (st, idx, mean_b, value_b, std, dmean, dvalue, out, a)


def test_loss_sums_are_published_to_the_last_workgroup(lib):
    check_publication(lambda seed, size: loss_case(lib, seed, size))


# ---------------------------------------------------------------------------------------------- adaptation MSE
def mse_case(lib, seed, size):
    rows = M if size == "full" else 10000
    npv = 2
    g = gen(20 + seed)
    target = torch.randn(R, npv, device="cuda", generator=g)
    idx = torch.randperm(R, device="cuda", generator=g)[:rows]
    pred = torch.zeros(rows, 64, device="cuda", dtype=torch.bfloat16)
    pred[:, :npv] = torch.randn(rows, npv, device="cuda", generator=g).to(torch.bfloat16)
    num_train = rows // 5 * 4
    d = torch.zeros(rows, 64, device="cuda", dtype=torch.bfloat16)
    out = torch.zeros(2 + npv, device="cuda")                     # train loss, test loss, bias gradient[npv]

    def launch():
        out.zero_()
        assert lib.go1ppo_mse(pred.data_ptr(), 64, target.data_ptr(), npv, idx.data_ptr(), rows, num_train, 0, d.data_ptr(),
                              out[2:].data_ptr(), out[0:].data_ptr(), out[1:].data_ptr(), stream()) == 0

    def check(r):
        e = pred[:, :npv].double() - target[idx].double()
        close(r[0], (e[:num_train] ** 2).mean(), 2e-4, 0.0, "train")
        close(r[1], (e[num_train:] ** 2).mean(), 2e-4, 0.0, "test")
        close(d[:num_train, :npv].double(), 2.0 * e[:num_train] / (num_train * npv), 8e-3, 1e-9, "d_pred")
        close(r[2:], d[:, :npv].double().sum(0), 1e-3, 1e-6, "bias")

    return launch, lambda: out.clone(), check, (target, idx, pred, d, out)


def test_mse_sums_are_published_to_the_last_workgroup(lib):
    check_publication(lambda seed, size: mse_case(lib, seed, size))


# ---------------------------------------------------------------------------------------------- GAE statistics
def gae_case(lib, seed, size):
    N = ENVS if size == "full" else 1000
    T = STEPS
    g = gen(30 + seed)
    rew = torch.randn(T, N, device="cuda", generator=g)
    dones = (torch.rand(T, N, device="cuda", generator=g) < 0.1).to(torch.uint8)
    values = torch.randn(T, N, device="cuda", generator=g)
    last = torch.randn(N, device="cuda", generator=g)
    ret, adv = torch.empty(T, N, device="cuda"), torch.empty(T, N, device="cuda")
    stats = torch.zeros(3, device="cuda", dtype=torch.float64)
    gamma, lam = 0.99, 0.95

    def launch():
        stats.zero_()
        assert lib.go1ppo_gae(rew.data_ptr(), dones.data_ptr(), values.data_ptr(), last.data_ptr(), T, N, gamma, lam, ret.data_ptr(),
                              adv.data_ptr(), stats.data_ptr(), stream()) == 0

    def check(r):
        a_ref, nxt, v64 = torch.zeros(T, N, device="cuda", dtype=torch.float64), last.double(), values.double()
        run = torch.zeros(N, device="cuda", dtype=torch.float64)
        for t in range(T - 1, -1, -1):
            alive = 1.0 - dones[t].double()
            run = rew[t].double() + alive * gamma * nxt - v64[t] + alive * gamma * lam * run
            a_ref[t], nxt = run, v64[t]
        close(adv, a_ref, 1e-4, 1e-5, "advantages")
        a64 = adv.double()                                        # the kernel's double sums of its own fp32 advantages
        close(r[0], a64.sum(), 1e-9, 1e-9 * float(a64.abs().sum()), "sum")
        close(r[1], (a64 * a64).sum(), 1e-9, 0.0, "sum of squares")

    return launch, lambda: stats[:2].clone(), check, (rew, dones, values, last, ret, adv, stats)


def test_gae_statistics_are_published_to_the_last_workgroup(lib):
    check_publication(lambda seed, size: gae_case(lib, seed, size))


# ---------------------------------------------------------------------------------------------- batched weight gradient, bias columns
@pytest.fixture(scope="module")
def ppo_wgrad_problems():
    """(rows, n, k, ld_dz, ld_h, has_bias, zero) of every problem in the PPO backward pass's batched weight-gradient launch, read
    from the plan the fused update records at 4096 envs x 24 steps"""
    from go1_gym_learn.ppo_cse.actor_critic import ActorCritic
    from go1_gym_learn.ppo_cse.ppo import PPO, PPO_Args
    saved = PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels, PPO_Args.use_hip_graphs
    PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels, PPO_Args.use_hip_graphs = True, True, False
    try:
        torch.manual_seed(0)
        alg = PPO(ActorCritic(70, 2, 2100, 12), device="cuda:0")
        alg.init_storage(ENVS, STEPS, [70], [2], [2100], [12])
        g = gen(1)
        for _ in range(STEPS):
            hist, priv = torch.randn(ENVS, 2100, device="cuda", generator=g), torch.randn(ENVS, 2, device="cuda", generator=g)
            alg.act(torch.randn(ENVS, 70, device="cuda", generator=g), priv, hist)
            alg.process_env_step(torch.randn(ENVS, device="cuda", generator=g), torch.zeros(ENVS, dtype=torch.uint8, device="cuda"),
                                 {"env_bins": torch.zeros(ENVS, device="cuda"), "time_outs": torch.zeros(ENVS, dtype=torch.bool, device="cuda")})
        alg.compute_returns(hist, priv)
        alg.update()
        torch.cuda.synchronize()
        plans = [v for k, v in alg._train_net._plans.items() if k[0] == "ppo"]
        assert plans
        _, _, _, rec, tn, _ = plans[0]
        assert tn
        probs = [(dz.shape[0], dz.shape[1], h.shape[1], dz.stride(0), h.stride(0), gb is not None, zero or (0, 0, 0))
                 for dz, h, gW, gb, zero in rec]
    finally:
        PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels, PPO_Args.use_hip_graphs = saved
    del alg
    torch.cuda.empty_cache()
    assert any(p[5] for p in probs) and all(p[0] == M for p in probs), probs
    return probs


def wgrad_case(lib, probs, seed, size):
    from go1_gym_learn.ppo_cse import fused
    rows = M if size == "full" else M // 2 - 64                   # another row count: other row chunks, another number of contributors
    g = gen(40 + seed)
    tab = (fused.WgradProblem * len(probs))()
    keep, biases = [], []
    for P, (_, n, k, ld_dz, ld_h, has_bias, zero) in zip(tab, probs):
        dz = torch.randn(rows, ld_dz, device="cuda", generator=g).to(torch.bfloat16)
        h = torch.randn(rows, ld_h, device="cuda", generator=g).to(torch.bfloat16)
        dW = torch.zeros(n, k, device="cuda")
        bias = torch.zeros(n, device="cuda") if has_bias else None
        P.dz, P.h, P.dW, P.bias_grad = dz.data_ptr(), h.data_ptr(), dW.data_ptr(), bias.data_ptr() if has_bias else None
        P.rows, P.ld_dz, P.ld_h, P.n, P.k, P.ldw = rows, ld_dz, ld_h, n, k, k
        P.zero_n, P.zero_k0, P.zero_k1 = zero
        P.partials, P.partial_stride = 16, n * k                  # placeholder: the plan depends on whether a problem has slabs
        keep.append((dz, h, dW))
        if has_bias:
            biases.append((bias, dz, n))
    total = lib.go1ppo_wgrad_tn_plan(tab, len(probs))
    assert total > 0
    for P in tab:
        ws = torch.zeros(-(-P.rows // P.chunk_rows), P.n * P.k, device="cuda")
        keep.append(ws)
        P.partials = ws.data_ptr()
    assert lib.go1ppo_wgrad_tn_plan(tab, len(probs)) == total
    dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
    keep.append(dev)

    def launch():
        for bias, _, _ in biases:
            bias.fill_(-2.0)
        assert lib.go1ppo_wgrad_tn_batched(dev.data_ptr(), len(probs), total, stream()) == 0

    def check(r):
        off = 0
        for bias, dz, n in biases:
            ref = dz[:, :n].double().sum(0) - 2.0
            close(r[off:off + n], ref, 1e-4, 2e-3 * rows ** 0.5, ("bias", n))
            off += n

    return launch, lambda: torch.cat([b for b, _, _ in biases]), check, (keep, biases)


def test_weight_gradient_bias_columns_are_published_to_the_last_workgroup(lib, ppo_wgrad_problems):
    check_publication(lambda seed, size: wgrad_case(lib, ppo_wgrad_problems, seed, size))
