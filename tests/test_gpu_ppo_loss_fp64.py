"""go1ppo_loss and go1ppo_mse (csrc/go1ppo.hip) against the float64 model of tests/ppo_loss_ref.py, on every load / store path and
reduction round of the two kernels; and the optional (null) outputs of those two and of their one-launch twins go1ppo_mlp2_tail_ppo /
go1ppo_mlp2_tail_mse (csrc/go1ppo_mlp.h).

Every buffer sits inside canaries (7.0 / 7), inputs are compared with their copies after the launch, the sums accumulate onto non-zero
destinations, and every case is launched twice on fresh copies: the second launch finds the ticket counter as the first left it.

Bounds (derived in ppo_loss_ref.py, none taken from what the kernels give):
  per-sample bf16 gradients  |got - ref| <= 2^-8 |ref| + atol, atol = 2^-22 (|a| + |mu|) / sigma^2 |dlogp| and its analogues;
  sums                       |got - ref| <= (n_add 2^-24 + eps) sum |term|, n_add = 6 + 4 + ceil(rows / 256), eps = 2e-4 for the losses,
                             the KL and d_std, 0 for the bias sums, whose terms are the kernel's own bf16 outputs.
A sum's destination starts at a quarter of sum |term| (alternating signs): the final `*dst + t` then rounds within the two additions that
n_add counts and the kernel does not make (the first wave and the first workgroup are added to an exact 0).
Each test prints its largest error-to-bound ratios (run with -s); profiles/ppo_loss_fp64.txt keeps the figures measured on an MI355X.
The gradients' ratios come close to 1 (0.996) by construction: rounding to bf16 (8 significant bits) alone errs by up to 2^-9 of the
binade's upper end, which is 2^-8 of a value at its lower end, so 2^-8 |ref| is the store's own worst case and what the fp32 evaluation
adds has to fit into atol and into the distance of the worst sample from a binade's lower end.  It does, at every case of the tables.

A `tie` case has samples with v - v_old exactly on -+clip: there the value gradient is the unclipped branch's (torch.max splits it onto
two identical paths), which a `>` in place of the kernel's `>=` turns into 0."""
import ctypes

import pytest
import torch

import ppo_loss_ref as P
from test_gpu_ppo_tail_fused import PAD, Buf, Net, arr, assert_nets_equal, bits, gen, ppo_case, same, stream

pytestmark = pytest.mark.gpu

LOSS_SUMS = ("surrogate_loss", "value_loss", "kl", "d_value_bias")        # slots 0 .. 3 of the sums' buffer; then d_std[A], d_mean_bias[A]
LOSS_OPTIONAL = LOSS_SUMS + ("d_std", "d_mean_bias")
RATIOS = {}


@pytest.fixture(scope="module")
def lib():
    from go1_gym_learn.ppo_cse import fused
    yield fused.load_library()
    for fam in sorted(RATIOS):
        print(f"\nppo_loss_fp64 family [{fam}]: " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(RATIOS[fam].items())), end="")
    print()


def note(family, case, **ratios):
    print(f"\nppo_loss_fp64 case [{family}] {case}: " + "  ".join(f"{k}={v:.3f}" for k, v in ratios.items()), end="")
    fam = RATIOS.setdefault(family, {})
    for k, v in ratios.items():
        fam[k] = max(fam.get(k, 0.0), v)


class Mat(Buf):
    """Buf whose matrix starts `off` elements past the buffer's 16-byte aligned place; columns the initial values do not cover hold the canary"""

    def __init__(self, rows, ld, init=None, off=0, flat=None):
        if flat is None:
            flat = torch.full((PAD + off + rows * ld + PAD,), 7.0, dtype=torch.bfloat16, device="cuda")
        assert flat.data_ptr() % 16 == 0
        self.flat, self.rows, self.ld, self.off = flat, rows, ld, off
        self.m = flat[PAD + off:PAD + off + rows * ld].view(rows, ld)
        if init is not None:
            self.m[:, :init.shape[1]] = init.to("cuda")

    def clone(self):
        return Mat(self.rows, self.ld, off=self.off, flat=self.flat.clone())

    def outside(self, cols):
        """everything but the first `cols` columns of the matrix: canaries and untouched columns, as one tensor"""
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        keep[PAD + self.off:PAD + self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :cols] = False
        return self.flat[keep]


class Vec:
    """the values of a CPU tensor, flattened, inside a canary-filled buffer of their type, `off` elements past its 16-byte aligned place"""

    def __init__(self, data=None, off=0, flat=None, n=None):
        if flat is None:
            n = data.numel()
            flat = torch.full((PAD + off + n + PAD,), 7, dtype=data.dtype, device="cuda")
            flat[PAD + off:PAD + off + n] = data.flatten().to("cuda")
        assert flat.data_ptr() % 16 == 0
        self.flat, self.off, self.n = flat, off, n
        self.v = flat[PAD + off:PAD + off + n]

    def clone(self):
        return Vec(off=self.off, flat=self.flat.clone(), n=self.n)

    def ptr(self):
        return self.v.data_ptr()

    def canaries_intact(self):
        return bool((self.flat[:PAD + self.off] == 7).all()) and bool((self.flat[PAD + self.off + self.n:] == 7).all())


def signed_quarter(abs_sums):
    """non-zero starting values of the sums' destinations: a quarter of sum |term|, signs alternating, in fp32"""
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(abs_sums.numel())[:abs_sums.numel()]
    return (0.25 * sign * abs_sums).float()


def worst(err, bound):
    """largest err / bound; a zero bound admits a zero error only"""
    bad = ~(err <= bound)                                         # a NaN is outside every bound
    assert not bool(bad.any()), f"{int(bad.sum())} of {err.numel()} outside their bound, worst ratio {float((err / bound)[bad].max()):.3f}"
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


# ------------------------------------------------------------------------------------------------------------------ go1ppo_loss
class LossRun:
    """device buffers of one loss case and what one launch on fresh copies of them leaves behind"""

    def __init__(self, c, d, dst0):
        self.c = c
        o = c.off
        self.mean = Mat(c.rows, c.head_ld, d["mean"], off=o.get("mean", 0))
        self.value = Mat(c.rows, c.head_ld, d["value"][:, None])
        self.std, self.idx = Vec(d["std"]), Vec(d["idx"])
        self.st = {k: Vec(t, off=o.get(k, 0)) for k, t in d["storage"].items()}
        self.d_mean, self.d_value = Mat(c.rows, c.head_ld, off=o.get("d_mean", 0)), Mat(c.rows, c.head_ld)
        self.sums = Vec(dst0)

    def inputs(self):
        return [("mean", self.mean), ("value", self.value), ("std", self.std), ("idx", self.idx)] + list(self.st.items())

    def launch(self, lib, null=()):
        from go1_gym_learn.ppo_cse import fused as F
        c, A = self.c, self.c.A
        d_mean, d_value, sums = self.d_mean.clone(), self.d_value.clone(), self.sums.clone()
        before = [(name, b, b.flat.clone()) for name, b in self.inputs()]
        a = F.LossArgs()
        a.mean, a.value, a.std, a.idx = self.mean.ptr(), self.value.ptr(), self.std.ptr(), self.idx.ptr()
        a.head_ld, a.num_actions, a.rows = c.head_ld, A, c.rows
        for k, t in self.st.items():
            setattr(a, k, None if (k == "old_values" and c.null_old_values) else t.ptr())
        a.clip_param, a.value_loss_coef, a.entropy_coef, a.use_clipped_value_loss = P.CLIP, P.VALUE_COEF, P.ENTROPY_COEF, c.clipped
        a.d_mean, a.d_value = d_mean.ptr(), d_value.ptr()
        for i, name in enumerate(LOSS_SUMS):
            setattr(a, name, sums.v[i:].data_ptr())
        a.d_std, a.d_mean_bias = sums.v[4:].data_ptr(), sums.v[4 + A:].data_ptr()
        for name in null:
            setattr(a, name, None)
        # the paths the case is in the table for are the ones the pointers select
        vec4 = A % 4 == 0 and c.head_ld % 4 == 0 and (a.actions | a.old_mu | a.old_sigma) % 16 == 0 and a.mean % 8 == 0
        fam = "scalar" if not vec4 else "vector loads, scalar stores" if a.d_mean % 8 else "wide heads" if A > 12 else "vector"
        assert fam == P.loss_family(c), (fam, P.loss_family(c))
        rc = lib.go1ppo_loss(ctypes.byref(a), stream())
        torch.cuda.synchronize()
        assert rc == 0
        for name, b, copy in before:
            assert same(b.flat, copy), f"input {name} was written"
        assert bool((d_mean.outside(A) == 7.0).all()), "d_mean: a canary or a column >= num_actions was written"
        assert bool((d_value.outside(1) == 7.0).all()), "d_value: a canary or a column >= 1 was written"
        assert sums.canaries_intact()
        return d_mean, d_value, sums


def loss_dst0(c, m):
    d_value_abs = m["d_value"].abs().sum().reshape(1)
    return signed_quarter(torch.cat([torch.tensor([m["surrogate_abs"], m["value_loss_abs"], m["kl_abs"]], dtype=torch.float64), d_value_abs,
                                     m["d_std_abs"], m["d_mean"].abs().sum(0)]))


@pytest.mark.parametrize("c", P.LOSS_CASES, ids=lambda c: c.name)
def test_loss_kernel_matches_the_fp64_model(lib, c):
    d = P.loss_inputs(c)
    m = P.loss_model(d)
    A, rows = c.A, c.rows
    dst0 = loss_dst0(c, m)
    run = LossRun(c, d, dst0)
    first = None
    for launch in (0, 1):
        d_mean, d_value, sums = run.launch(lib)
        got_mean, got_value, got = d_mean.m[:, :A].double().cpu(), d_value.m[:, 0].double().cpu(), sums.v.double().cpu()
        r_mean = worst((got_mean - m["d_mean"]).abs(), P.grad_bound(m["d_mean"], m["d_mean_atol"]))
        r_value = worst((got_value - m["d_value"]).abs(), P.grad_bound(m["d_value"], m["d_value_atol"]))
        # the three losses' sums, the KL and d_std (entropy term included)
        ref = torch.cat([torch.tensor([m["surrogate"], m["value_loss"], m["kl"]], dtype=torch.float64), m["d_std"]])
        abs_sum = torch.cat([torch.tensor([m["surrogate_abs"], m["value_loss_abs"], m["kl_abs"]], dtype=torch.float64), m["d_std_abs"]])
        pick = [0, 1, 2] + list(range(4, 4 + A))
        r_sums = worst((got[pick] - (dst0.double()[pick] + ref)).abs(), P.sum_bound(rows, abs_sum, 2e-4))
        # the bias sums: float64 sums of the kernel's own outputs
        pick = [3] + list(range(4 + A, 4 + 2 * A))
        ref = torch.cat([got_value.sum().reshape(1), got_mean.sum(0)])
        abs_sum = torch.cat([got_value.abs().sum().reshape(1), got_mean.abs().sum(0)])
        r_bias = worst((got[pick] - (dst0.double()[pick] + ref)).abs(), P.sum_bound(rows, abs_sum, 0.0))
        if launch == 0:
            first = (d_mean, d_value, sums)
            note(P.loss_family(c), c.name, d_mean=r_mean, d_value=r_value, sums=r_sums, bias_sums=r_bias)
        else:
            for name, x, y in zip(("d_mean", "d_value", "sums"), (d_mean, d_value, sums), first):
                assert same(x.flat, y.flat), f"launch 1: {name} differs from launch 0"
    if c.tie:
        # on the edge the value gradient is the unclipped branch's: a kernel that counted the edge as outside would store 0 here
        k = int(d["tie_rows"].sum())
        assert bool((first[1].m[:k, 0].float().abs().cpu() > 0).all()) and bool((m["d_value"][:k].abs() > 1e-4 / rows).all())


# ------------------------------------------------------------------------------------------------------------------ go1ppo_mse
class MseRun:
    def __init__(self, c, d, dst0):
        self.c = c
        self.pred, self.d_pred = Mat(c.rows, c.pred_ld, d["pred"]), Mat(c.rows, c.pred_ld)
        self.target, self.idx = Vec(d["target"]), Vec(d["idx"])
        self.sums = Vec(dst0)                                     # [train, test, d_pred_bias[npv]]

    def launch(self, lib, null_bias=False):
        c = self.c
        d_pred, sums = self.d_pred.clone(), self.sums.clone()
        before = [(name, b, b.flat.clone()) for name, b in (("pred", self.pred), ("target", self.target), ("idx", self.idx))]
        rc = lib.go1ppo_mse(self.pred.ptr(), c.pred_ld, self.target.ptr(), c.npv, self.idx.ptr(), c.rows, c.num_train, c.selective, d_pred.ptr(),
                            None if null_bias else sums.v[2:].data_ptr(), sums.v[0:].data_ptr(), sums.v[1:].data_ptr(), stream())
        torch.cuda.synchronize()
        assert rc == 0
        for name, b, copy in before:
            assert same(b.flat, copy), f"input {name} was written"
        assert bool((d_pred.outside(c.npv) == 7.0).all()), "d_pred: a canary or a column >= npv was written"
        assert sums.canaries_intact()
        return d_pred, sums


def mse_dst0(c, m):
    dst0 = signed_quarter(torch.cat([torch.tensor([m["train_loss"], m["test_loss"]], dtype=torch.float64), m["d_pred"].abs().sum(0)]))
    dst0[2 + (1 if c.selective else c.npv):] = 0.31               # bias columns the selective loss never reaches: to be left as they are
    return dst0


@pytest.mark.parametrize("c", P.MSE_CASES, ids=lambda c: c.name)
def test_mse_kernel_matches_the_fp64_model(lib, c):
    d = P.mse_inputs(c)
    m = P.mse_model(d)
    ncol = 1 if c.selective else c.npv
    dst0 = mse_dst0(c, m)
    run = MseRun(c, d, dst0)
    first = None
    for launch in (0, 1):
        d_pred, sums = run.launch(lib)
        g, got = d_pred.m[:, :c.npv].double().cpu(), sums.v.double().cpu()
        r_grad = worst((g - m["d_pred"]).abs(), P.grad_bound(m["d_pred"], m["d_pred_atol"]))
        # what carries no gradient is an exact (positive) zero
        assert not bits(d_pred.m[c.num_train:, :c.npv]).any() and not bits(d_pred.m[:, ncol:c.npv]).any()
        loss_abs = torch.tensor([m["train_loss"], m["test_loss"]], dtype=torch.float64)
        r_loss = worst((got[:2] - (dst0.double()[:2] + loss_abs)).abs(), P.sum_bound(c.rows, loss_abs, 2e-4))
        r_bias = worst((got[2:2 + ncol] - (dst0.double()[2:2 + ncol] + g[:, :ncol].sum(0))).abs(), P.sum_bound(c.rows, g[:, :ncol].abs().sum(0), 0.0))
        assert torch.equal(sums.v[2 + ncol:].cpu(), dst0[2 + ncol:])
        if launch == 0:
            first = (d_pred, sums)
            note(P.mse_family(c), c.name, d_pred=r_grad, losses=r_loss, bias_sums=r_bias)
        else:
            assert same(d_pred.flat, first[0].flat) and same(sums.flat, first[1].flat), "launch 1 differs from launch 0"


# ------------------------------------------------------------------------------------------------------------------ null outputs
NULL_SETS = [(name,) for name in LOSS_OPTIONAL] + [LOSS_OPTIONAL]


def loss_slots(name, A):
    return {"d_std": range(4, 4 + A), "d_mean_bias": range(4 + A, 4 + 2 * A)}.get(name) or [LOSS_SUMS.index(name)]


@pytest.mark.parametrize("A", [12, 5])
def test_loss_kernel_null_outputs(lib, A):
    """each optional sum absent alone, then all of them: 0, that destination untouched, every other output as with all present"""
    c = P._lc(f"null-A{A}", 257, A)
    d = P.loss_inputs(c)
    dst0 = loss_dst0(c, P.loss_model(d))
    run = LossRun(c, d, dst0)
    base = run.launch(lib)
    for null in NULL_SETS:
        for launch in (0, 1):
            d_mean, d_value, sums = run.launch(lib, null)
            assert same(d_mean.flat, base[0].flat) and same(d_value.flat, base[1].flat), (null, launch)
            absent = sorted(i for name in null for i in loss_slots(name, A))
            present = [i for i in range(4 + 2 * A) if i not in absent]
            assert same(sums.v[absent], run.sums.v[absent]), (null, launch, "an absent output's place was written")
            assert same(sums.v[present], base[2].v[present]), (null, launch)
            assert not same(base[2].v[absent], run.sums.v[absent])


@pytest.mark.parametrize("npv", [2, 7])
def test_mse_kernel_null_bias(lib, npv):
    c = P.MseCase(f"null-npv{npv}", 257, 205, npv, 0, 64)
    d = P.mse_inputs(c)
    run = MseRun(c, d, mse_dst0(c, P.mse_model(d)))
    base = run.launch(lib)
    for launch in (0, 1):
        d_pred, sums = run.launch(lib, null_bias=True)
        assert same(d_pred.flat, base[0].flat), launch
        assert same(sums.v[:2], base[1].v[:2]) and same(sums.v[2:], run.sums.v[2:]) and not same(base[1].v[2:], run.sums.v[2:]), launch


@pytest.mark.parametrize("A", [12, 5])
def test_ppo_tail_null_outputs(lib, A):
    """go1ppo_mlp2_tail_ppo: as above; the nets' buffers (x, z2, the heads, d_out, d_z2, d_x, canaries included) bit for bit as well"""
    (o_actor, o_critic, d_ref), fused_run = ppo_case(lib, 257, A, 1)
    rc, b_actor, b_critic, b_d = fused_run()
    assert rc == 0
    place = {"value_loss": (0, 0), "surrogate_loss": (0, 1), "kl": (0, 2), "d_value_bias": (0, 3), "d_std": (1, None), "d_mean_bias": (2, None)}
    start = (torch.arange(1, 5, device="cuda", dtype=torch.float32) * 0.37, torch.full((A,), 0.11, device="cuda"), torch.full((A,), -0.23, device="cuda"))
    for null in NULL_SETS:
        for launch in (0, 1):
            rc, a, c, d = fused_run(null)
            assert rc == 0
            assert_nets_equal(a, b_actor, f"actor, {null}, launch {launch}")
            assert_nets_equal(c, b_critic, f"critic, {null}, launch {launch}")
            want = [t.clone() for t in b_d]
            for name in null:
                t, i = place[name]
                if i is None:
                    want[t] = start[t]
                else:
                    want[t][i] = start[t][i]
            for x, y in zip(d, want):
                assert same(x, y), (null, launch, x.tolist(), y.tolist())


@pytest.mark.parametrize("npv", [2, 7])
def test_mse_tail_null_bias(lib, npv):
    from go1_gym_learn.ppo_cse import fused as F
    rows, num_train = 257, 205
    g = gen(31 * npv)
    net = Net(rows, g)
    S = 2 * rows + 3
    idx = torch.randperm(S, device="cuda", generator=g)[:rows].contiguous()
    target = torch.randn(S, npv, device="cuda", generator=g)
    results = []
    for null in (False, True, True):
        f, fb, fl = net.clone(), torch.full((npv,), 0.31, device="cuda"), torch.tensor([0.5, -0.25], device="cuda")
        q = F.MseArgs()
        q.target, q.idx, q.num_train, q.npv, q.selective = target.data_ptr(), idx.data_ptr(), num_train, npv, 0
        q.d_pred_bias, q.train_loss, q.test_loss = None if null else fb.data_ptr(), fl[0:].data_ptr(), fl[1:].data_ptr()
        assert lib.go1ppo_mlp2_tail_mse(arr(F.Mlp2Tail, [f.tail(F)]), ctypes.byref(q), stream()) == 0
        torch.cuda.synchronize()
        results.append((f, fb, fl))
    base = results[0]
    assert bool((base[1] != 0.31).all())
    for f, fb, fl in results[1:]:
        assert_nets_equal(f, base[0], "null d_pred_bias")
        assert same(fl, base[2]) and bool((fb == 0.31).all())
