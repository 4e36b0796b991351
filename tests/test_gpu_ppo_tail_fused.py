"""go1ppo_mlp2_tail_ppo / go1ppo_mlp2_tail_mse (csrc/go1ppo_mlp.h): forward, loss and backward of the 256 -> 128 -> 64 MLP ends as ONE
launch per pass.  The oracle is the three launches they replace (go1ppo_mlp2_fwd, go1ppo_loss or go1ppo_mse, go1ppo_mlp2_bwd) on copies of
the same buffers, and every comparison is bit for bit (torch.equal on the raw bits, canaries around every buffer included): the activated
x, z2, the head, d_out, d_z2, d_x, and every sum — losses, KL, d_std, the bias gradients — accumulated onto non-zero destinations.

Row counts: 1 (a partial tile), 64 (an exact tile), 65 (a tile edge), 257 (a 256-row group of the sums plus a row: the 4-tile combination
and the partial last group), 8259 (130 tiles on 128 workgroups per net: the tile walk and the prefetch take a second round; no multiple
of 64 or 256); the adaptation tail also 16449 rows (258 tiles on its 256 workgroups).  Every case is launched twice on fresh copies of the
inputs: the second launch finds the ticket counter as the first left it."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 512                       # canary elements in front of and behind every buffer
LDX, LDZ, HEAD = 264, 136, 64   # leading dimensions: padded rows for the 256- and 128-wide matrices; the heads are 64 wide


@pytest.fixture(scope="module")
def lib():
    from go1_gym_learn.ppo_cse import fused
    return fused.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


class Buf:
    """(rows x ld) bf16 matrix inside a canary-filled flat buffer"""

    def __init__(self, rows, ld, init=None, flat=None):
        if flat is None:
            flat = torch.full((PAD + rows * ld + PAD,), 7.0, dtype=torch.bfloat16, device="cuda")
            if init is not None:
                flat[PAD:PAD + rows * ld].view(rows, ld)[:, :init.shape[1]] = init
        self.flat, self.rows, self.ld = flat, rows, ld
        self.m = flat[PAD:PAD + rows * ld].view(rows, ld)

    def clone(self):
        return Buf(self.rows, self.ld, flat=self.flat.clone())

    def ptr(self):
        return self.m.data_ptr()


class Net:
    """weights and buffers of one 256 -> 128 -> 64 end; d_out starts with non-zero values in every column"""

    def __init__(self, rows, g):
        r = lambda *s, scale=1.0: (torch.randn(*s, device="cuda", generator=g) * scale).to(torch.bfloat16)
        self.rows = rows
        self.W2, self.b2, self.W3, self.b3 = r(128, 256, scale=1 / 16), r(128, scale=0.1), r(64, 128, scale=1 / 11), r(64, scale=0.1)
        self.x = Buf(rows, LDX, r(rows, 256, scale=1.5))
        self.z2, self.dz2 = Buf(rows, LDZ), Buf(rows, LDZ)
        self.out, self.dout = Buf(rows, HEAD), Buf(rows, HEAD, r(rows, 64, scale=0.01))
        self.dx = Buf(rows, LDX)

    def clone(self):
        n = object.__new__(Net)
        n.__dict__.update(self.__dict__)
        for k in ("x", "z2", "dz2", "out", "dout", "dx"):
            setattr(n, k, getattr(self, k).clone())
        return n

    def bufs(self):
        return [("x", self.x), ("z2", self.z2), ("out", self.out), ("d_out", self.dout), ("d_z2", self.dz2), ("d_x", self.dx)]

    def fwd(self, F):
        a = F.Mlp2Fwd()
        a.x, a.W2, a.b2, a.W3, a.b3 = self.x.ptr(), self.W2.data_ptr(), self.b2.data_ptr(), self.W3.data_ptr(), self.b3.data_ptr()
        a.z2, a.out, a.rows, a.ld_x, a.ld_z2, a.ld_out, a.elu_input = self.z2.ptr(), self.out.ptr(), self.rows, LDX, LDZ, HEAD, 1
        return a

    def bwd(self, F):
        a = F.Mlp2Bwd()
        a.d_out, a.z2, a.h, a.W2, a.W3 = self.dout.ptr(), self.z2.ptr(), self.x.ptr(), self.W2.data_ptr(), self.W3.data_ptr()
        a.d_z2, a.d_x, a.rows = self.dz2.ptr(), self.dx.ptr(), self.rows
        a.ld_dout, a.ld_z2, a.ld_h, a.ld_dz2, a.ld_dx = HEAD, LDZ, LDX, LDZ, LDX
        return a

    def tail(self, F):
        a = F.Mlp2Tail()
        a.x, a.W2, a.b2, a.W3, a.b3 = self.x.ptr(), self.W2.data_ptr(), self.b2.data_ptr(), self.W3.data_ptr(), self.b3.data_ptr()
        a.z2, a.out, a.d_out, a.d_z2, a.d_x, a.rows = self.z2.ptr(), self.out.ptr(), self.dout.ptr(), self.dz2.ptr(), self.dx.ptr(), self.rows
        a.ld_x, a.ld_z2, a.ld_out, a.ld_dout, a.ld_dz2, a.ld_dx, a.elu_input = LDX, LDZ, HEAD, HEAD, LDZ, LDX, 1
        return a


def arr(cls, items):
    a = (cls * len(items))()
    for i, it in enumerate(items):
        ctypes.memmove(ctypes.byref(a[i]), ctypes.byref(it), ctypes.sizeof(cls))
    return a


def assert_nets_equal(got, want, what):
    for (name, a), (_, b) in zip(got.bufs(), want.bufs()):
        assert same(a.flat, b.flat), f"{what}: {name} differs in {int((bits(a.flat) != bits(b.flat)).sum())} elements"


# ------------------------------------------------------------------------------------------------------------------ PPO
def ppo_case(lib, rows, A, clipped):
    """inputs, the oracle's results, and a function that runs the fused launch on fresh copies"""
    from go1_gym_learn.ppo_cse import fused as F
    g = gen(1000 * A + 10 * rows + clipped)
    actor, critic = Net(rows, g), Net(rows, g)
    S = 2 * rows + 7                                               # the storage is larger than the mini-batch; idx is a permuted subset
    idx = torch.randperm(S, device="cuda", generator=g)[:rows].contiguous()
    std = torch.rand(A, device="cuda", generator=g) * 0.5 + 0.5
    # storage values that put the ratio and the value difference on both sides of their clip ranges: a forward pass of the oracle first
    o_actor, o_critic = actor.clone(), critic.clone()
    assert lib.go1ppo_mlp2_fwd(arr(F.Mlp2Fwd, [o_actor.fwd(F), o_critic.fwd(F)]), 2, stream()) == 0
    mean, value = o_actor.out.m[:, :A].float(), o_critic.out.m[:, 0].float()
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    st = {k: rnd(S, A) for k in ("actions", "old_mu")}
    st["old_sigma"] = torch.rand(S, A, device="cuda", generator=g) * 0.5 + 0.5
    st.update({k: rnd(S) for k in ("old_logp", "advantages", "returns", "old_values")})
    noise = rnd(rows, A)
    st["actions"][idx] = mean + std * noise
    st["old_mu"][idx] = mean + 0.1 * rnd(rows, A)
    logp = (-0.5 * noise * noise - torch.log(std) - 0.9189385332046727).sum(1)
    st["old_logp"][idx] = logp + 0.3 * rnd(rows)
    st["old_values"][idx] = value + 0.3 * rnd(rows)
    st["returns"][idx] = value + rnd(rows)

    def dests():
        # [value_loss, surrogate, kl, d_value_bias], d_std, d_mean_bias: non-zero, so that the sums are seen to be ADDED
        return torch.arange(1, 5, device="cuda", dtype=torch.float32) * 0.37, torch.full((A,), 0.11, device="cuda"), torch.full((A,), -0.23, device="cuda")

    def loss_args(a_net, c_net, d):
        a = F.LossArgs()
        a.mean, a.value, a.std, a.head_ld, a.num_actions, a.rows, a.idx = a_net.out.ptr(), c_net.out.ptr(), std.data_ptr(), HEAD, A, rows, idx.data_ptr()
        for k, t in st.items():
            setattr(a, k, t.data_ptr())
        a.clip_param, a.value_loss_coef, a.entropy_coef, a.use_clipped_value_loss = 0.2, 1.0, 0.01, clipped
        a.d_mean, a.d_value, a.d_std, a.d_mean_bias = a_net.dout.ptr(), c_net.dout.ptr(), d[1].data_ptr(), d[2].data_ptr()
        a.value_loss, a.surrogate_loss, a.kl, a.d_value_bias = d[0][0:].data_ptr(), d[0][1:].data_ptr(), d[0][2:].data_ptr(), d[0][3:].data_ptr()
        return a

    d_ref = dests()
    la = loss_args(o_actor, o_critic, d_ref)
    assert lib.go1ppo_loss(ctypes.byref(la), stream()) == 0
    assert lib.go1ppo_mlp2_bwd(arr(F.Mlp2Bwd, [o_actor.bwd(F), o_critic.bwd(F)]), 2, stream()) == 0
    torch.cuda.synchronize()

    def fused_run(null=()):
        a, c, d = actor.clone(), critic.clone(), dests()
        la = loss_args(a, c, d)
        for name in null:                                          # optional outputs passed as null pointers
            setattr(la, name, None)
        rc = lib.go1ppo_mlp2_tail_ppo(arr(F.Mlp2Tail, [a.tail(F), c.tail(F)]), ctypes.byref(la), stream())
        torch.cuda.synchronize()
        return rc, a, c, d

    return (o_actor, o_critic, d_ref), fused_run


# A = 1, 4 and 9: the AMAX = 4 instantiation, its 16-byte gathers (A = 4), and a head that is no multiple of 4 in the AMAX = 12 one
PPO_CASES = [(rows, A, clipped) for clipped in (1, 0) for A in (12, 5) for rows in (1, 64, 65, 257, 8259)] + \
            [(rows, A, clipped) for clipped in (1, 0) for A in (1, 4, 9) for rows in (65, 257)]


@pytest.mark.parametrize("rows,A,clipped", PPO_CASES)
def test_ppo_tail_equals_three_launches(lib, rows, A, clipped):
    (o_actor, o_critic, d_ref), fused_run = ppo_case(lib, rows, A, clipped)
    assert all(bool(torch.isfinite(t).all()) for t in d_ref)
    for launch in (0, 1):
        rc, a, c, d = fused_run()
        assert rc == 0
        assert_nets_equal(a, o_actor, f"actor, launch {launch}")
        assert_nets_equal(c, o_critic, f"critic, launch {launch}")
        for name, x, y in zip(("losses / kl / d_value_bias", "d_std", "d_mean_bias"), d, d_ref):
            assert same(x, y), (launch, name, x.tolist(), y.tolist())


def test_ppo_tail_refuses_wide_heads(lib):
    """num_actions above GO1PPO_TAIL_MAX_ACTIONS: -1 and nothing written (such heads keep the three launches)"""
    (o_actor, _, _), fused_run = ppo_case(lib, 65, 16, 1)
    rc, a, c, d = fused_run()
    assert rc == -1
    assert bool((a.out.flat == 7.0).all()) and bool((a.dx.flat == 7.0).all()) and bool((c.dz2.flat == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------ MSE
def num_train_cases(rows):
    """a tile edge, inside a tile, and the update's rows // 5 * 4 — those that leave both parts non-empty"""
    edge = 64 * max(1, (rows // 2) // 64)
    out = []
    for n in (edge, edge + 17 if rows > 100 else rows // 2, rows // 5 * 4):
        if 0 < n < rows and n not in out:
            out.append(n)
    return out


MSE_CASES = [(rows, n) for rows in (2, 64, 65, 257, 8259, 16449) for n in num_train_cases(rows)]
# npv = 2 as the policy has it; then widths whose targets pass the 8 gathered ahead and whose head columns reach the second 16-byte chunk
MSE_PARAMS = [pytest.param(rows, n, selective, 2, id=f"{rows}-{n}-{selective}") for selective in (0, 1) for rows, n in MSE_CASES] + \
             [pytest.param(rows, n, selective, npv, id=f"{rows}-{n}-{selective}-npv{npv}") for selective in (0, 1) for npv in (1, 7, 9, 13, 64)
              for rows in (65, 257) for n in num_train_cases(rows)[1:]]


@pytest.mark.parametrize("rows,num_train,selective,npv", MSE_PARAMS)
def test_mse_tail_equals_three_launches(lib, rows, num_train, selective, npv):
    from go1_gym_learn.ppo_cse import fused as F
    g = gen(7 * rows + num_train + selective)
    net = Net(rows, g)
    S = 2 * rows + 3
    idx = torch.randperm(S, device="cuda", generator=g)[:rows].contiguous()
    target = torch.randn(S, npv, device="cuda", generator=g)
    dests = lambda: (torch.full((npv,), 0.31, device="cuda"), torch.tensor([0.5, -0.25], device="cuda"))
    o, (ob, ol) = net.clone(), dests()
    assert lib.go1ppo_mlp2_fwd(arr(F.Mlp2Fwd, [o.fwd(F)]), 1, stream()) == 0
    assert lib.go1ppo_mse(o.out.ptr(), HEAD, target.data_ptr(), npv, idx.data_ptr(), rows, num_train, selective, o.dout.ptr(), ob.data_ptr(),
                          ol[0:].data_ptr(), ol[1:].data_ptr(), stream()) == 0
    assert lib.go1ppo_mlp2_bwd(arr(F.Mlp2Bwd, [o.bwd(F)]), 1, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ol).all()) and float(ol[0]) != 0.5 and float(ol[1]) != -0.25
    for launch in (0, 1):
        f, (fb, fl) = net.clone(), dests()
        q = F.MseArgs()
        q.target, q.idx, q.num_train, q.npv, q.selective = target.data_ptr(), idx.data_ptr(), num_train, npv, selective
        q.d_pred_bias, q.train_loss, q.test_loss = fb.data_ptr(), fl[0:].data_ptr(), fl[1:].data_ptr()
        assert lib.go1ppo_mlp2_tail_mse(arr(F.Mlp2Tail, [f.tail(F)]), ctypes.byref(q), stream()) == 0
        torch.cuda.synchronize()
        assert_nets_equal(f, o, f"launch {launch}")
        assert same(fb, ob), (launch, fb.tolist(), ob.tolist())
        assert same(fl, ol), (launch, fl.tolist(), ol.tolist())


# --------------------------------------------------------------------------------------------------------------- engine
def test_engine_wiring_equals_the_three_launches(monkeypatch):
    """FusedNet at 320 rows on the large-batch engine: the PPO stage and the adaptation stage through the one-launch wiring against the same
    stages with the old calls — flat fp32 gradient, loss accumulators and KL bit for bit"""
    from go1_gym_learn.ppo_cse.actor_critic import ActorCritic
    from go1_gym_learn.ppo_cse.fused import FusedNet
    from go1_gym_learn.ppo_cse.ppo import PPO, PPO_Args
    monkeypatch.setenv("GO1_FUSED_TAILS_MAX_ROWS", "0")
    N, T, mb = 80, 8, 320
    keep = PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels
    PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels = True, True
    try:
        torch.manual_seed(0)
        alg = PPO(ActorCritic(70, 2, 2100, 12), device="cuda:0")
        alg.init_storage(N, T, [70], [2], [2100], [12])
        g = gen(3)
        for t in range(T):
            obs, priv, hist = (torch.randn(N, k, device="cuda", generator=g) for k in (70, 2, 2100))
            torch.manual_seed(100 + t)
            alg.act(obs, priv, hist)
            alg.process_env_step(torch.randn(N, device="cuda", generator=g), torch.zeros(N, dtype=torch.uint8, device="cuda"),
                                 {"env_bins": torch.zeros(N, device="cuda"), "time_outs": torch.zeros(N, dtype=torch.bool, device="cuda")})
        alg.compute_returns(hist, priv)
        idx = torch.randperm(N * T, device="cuda", generator=g)[:mb]
        net = alg._train_net = FusedNet(alg.policy, alg.body, alg.master.grad[:alg.n_body], mb, alg._fused_lib, with_grad=True)
        assert net._mlp2 and net.tail_ppo_fused(12) and net.tail_adaptation_fused()
        st, n = alg.storage, alg.n_body
        num_train = mb // 5 * 4

        def old_ppo():
            alg._gather_rows(idx, net.X)
            net.forward(net.X)
            net.ppo_loss(st, idx, alg.std, alg.master.grad[n:n + alg.n_std], PPO_Args, alg._kl, alg._acc)
            net.backward(net.X)

        def old_adapt():
            net.forward_adaptation(net.X)
            net.adaptation_loss(st, idx, num_train, PPO_Args.selective_adaptation_module_loss, alg._acc)
            net.backward_adaptation(net.X)

        results = []
        for stages in ((lambda: alg._stage_ppo_backward(idx), lambda: alg._stage_adapt_backward(idx)), (old_ppo, old_adapt)):
            per_stage = []
            for stage in stages:
                alg.master.grad.zero_()
                alg._acc.zero_()
                alg._kl.zero_()
                with torch.no_grad():
                    stage()
                torch.cuda.synchronize()
                per_stage.append((alg.master.grad.clone(), alg._acc.clone(), alg._kl.clone()))
            results.append(per_stage)
        for what, new, old in zip(("ppo", "adaptation"), *results):
            assert float(old[0].abs().sum()) > 0
            for name, a, b in zip(("gradient", "loss accumulators", "kl"), new, old):
                assert same(a, b), (what, name, int((bits(a) != bits(b)).sum()))
    finally:
        PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels = keep
