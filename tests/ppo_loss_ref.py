"""float64 model of the PPO loss stage (go1ppo_loss, go1ppo_mlp2_tail_ppo) and of the adaptation regression (go1ppo_mse,
go1ppo_mlp2_tail_mse), the recipe that builds their test inputs, and the tables of cases the CPU and the GPU tests share.

The model is plain torch on the CPU, written from the statements of go1_gym_learn/ppo_cse/ppo.py (Normal log-probability and entropy,
the KL expression, the surrogate, the clipped or plain value loss, F.mse_loss on the train and test rows); every gradient is float64
autograd of the total loss.  It reads the bits the kernels read: the bf16 head outputs widened exactly, the fp32 storage gathered through
idx, clip_param as the fp32 number the argument struct carries.

A decision edge is a place where the formulas branch: ratio against 1 -+ clip, v - v_old against -+clip, and, outside the value clip,
the larger of the two squared errors.  fp32 and fp64 can fall on different sides of an edge, so the recipe moves every sample that lies
near one away from it (`repair`) and the tests assert that none is left inside the margins.  Samples of a `tie` case are put EXACTLY on a
value-clip edge instead (v = 0, v_old = -+clip: v - v_old is exact in both precisions): there the formulas' tie rule is what is tested."""
import math
from collections import namedtuple

import numpy as np
import torch

CLIP = float(np.float32(0.2))               # PPO_Args.clip_param as the kernels receive it
VALUE_COEF, ENTROPY_COEF = 1.0, 0.01
RATIO_MARGIN, VCLIP_MARGIN, BRANCH_MARGIN = 2e-3, 1e-3, 1e-2      # relative, absolute, relative
TIES = 8                                    # samples of a tie case that sit on an edge (fewer when the case has fewer rows)
_STORAGE = ("actions", "old_mu", "old_sigma", "old_logp", "advantages", "returns", "old_values")

LossCase = namedtuple("LossCase", "name rows A clipped head_ld off null_old_values tie")
MseCase = namedtuple("MseCase", "name rows num_train npv selective pred_ld")


def _lc(name, rows, A, clipped=1, head_ld=64, off=None, null_old_values=False, tie=False):
    return LossCase(name, rows, A, clipped, head_ld, dict(off or {}), null_old_values, tie)


# `off`: elements by which a pointer is moved off its 16-byte aligned place (fp32 elements for the storage, bf16 for mean / d_mean)
# (the two one-row cases are named so that their one sample has a gradient in the model: a clipped sample would compare 0 with 0)
LOSS_CASES = [_lc(f"rows{r}" if r > 1 else "row1", r, 12) for r in (1, 64, 65, 256, 257, 1031, 8259)] + \
             [_lc(f"A{A}", 257, A) for A in (1, 4, 5, 8, 16, 32)] + [
    _lc("A1-one-row", 1, 1),
    _lc("A5-rows1031", 1031, 5),
    _lc("A5-plain", 65, 5, clipped=0),
    _lc("A12-plain", 257, 12, clipped=0),
    _lc("A12-plain-no-old-values", 65, 12, clipped=0, null_old_values=True),
    _lc("A32-plain", 1031, 32, clipped=0),
    _lc("ld36", 257, 12, head_ld=36),
    _lc("ld34", 257, 12, head_ld=34),
    _lc("A5-ld36", 65, 5, head_ld=36),
    _lc("A32-ld36", 257, 32, head_ld=36),
    _lc("A32-ld34", 65, 32, head_ld=34),
    _lc("actions+1", 257, 12, off=dict(actions=1)),
    _lc("old_mu+1", 65, 12, off=dict(old_mu=1)),
    _lc("old_sigma+1", 257, 12, off=dict(old_sigma=1)),
    _lc("mean+2", 257, 12, off=dict(mean=2)),
    _lc("mean+4", 257, 12, off=dict(mean=4)),                    # 8-byte aligned, not 16: the vector path stays on
    _lc("d_mean+2", 257, 12, off=dict(d_mean=2)),                # vector loads, element stores
    _lc("d_mean+4", 65, 12, off=dict(d_mean=4)),
    _lc("A16-d_mean+2", 257, 16, off=dict(d_mean=2)),
    _lc("tie-A5", 65, 5, tie=True),
    _lc("tie-A12", 257, 12, tie=True),
    _lc("tie-A12-scalar", 65, 12, off=dict(actions=1), tie=True),
]

MSE_CASES = [MseCase(f"npv{n}", 257, 128, n, 0, 64) for n in (1, 2, 6, 7, 9, 13, 64)] + \
            [MseCase(f"npv{n}-selective", 257, 256, n, 1, 64) for n in (1, 2, 7, 64)] + [
    MseCase("two-rows", 2, 1, 2, 0, 64),
    MseCase("two-rows-selective", 2, 1, 7, 1, 64),
    MseCase("one-train-row", 257, 1, 9, 0, 64),
    MseCase("one-train-row-selective", 257, 1, 2, 1, 72),
    MseCase("one-test-row-npv13-ld72", 257, 256, 13, 0, 72),
    MseCase("rows1000-npv2", 1000, 800, 2, 0, 64),
    MseCase("rows1000-npv13-ld72", 1000, 800, 13, 0, 72),
    MseCase("rows1000-npv64-ld72", 1000, 800, 64, 0, 72),
    MseCase("rows1000-npv6-selective-ld72", 1000, 800, 6, 1, 72),
]


def loss_family(c):
    """which load / store path of loss_kernel the case takes"""
    o = c.off
    vec4 = c.A % 4 == 0 and c.head_ld % 4 == 0 and not any(o.get(k, 0) % 4 for k in ("actions", "old_mu", "old_sigma")) and o.get("mean", 0) % 4 == 0
    if not vec4:
        return "scalar"
    if o.get("d_mean", 0) % 4:
        return "vector loads, scalar stores"
    return "wide heads" if c.A > 12 else "vector"


def mse_family(c):
    ncol = 1 if c.selective else c.npv
    return "MSE, %s" % ("one round" if ncol <= 6 else "two rounds" if ncol <= 12 else "three or more rounds")


# ------------------------------------------------------------------------------------------------------------------ inputs
def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def _log_prob(a, mu, sg):
    return (-((a - mu) ** 2) / (2 * sg ** 2) - torch.log(sg) - math.log(math.sqrt(2 * math.pi))).sum(-1)


def edge_distances(d):
    """per sample, float64: relative distance of the ratio to the nearer of 1 -+ clip; distance of v - v_old to the nearer of -+clip; and
    |l1 - l2| / max(l1, l2) where the value difference is outside the clip (inf inside); `side`s: which side of each clip"""
    idx, st = d["idx"], d["storage"]
    mu, v, sg = d["mean"].double(), d["value"].double(), d["std"].double()
    logp = _log_prob(st["actions"][idx].double(), mu, sg)
    ratio = torch.exp(logp - st["old_logp"][idx].double())
    lo, hi = 1.0 - CLIP, 1.0 + CLIP
    r_dist = torch.minimum((ratio - lo).abs() / lo, (ratio - hi).abs() / hi)
    dlt = v - st["old_values"][idx].double()
    v_dist = torch.minimum((dlt - CLIP).abs(), (dlt + CLIP).abs())
    outside = dlt.abs() > CLIP
    R = st["returns"][idx].double()
    l1, l2 = (v - R) ** 2, (st["old_values"][idx].double() + dlt.clamp(-CLIP, CLIP) - R) ** 2
    b_dist = torch.where(outside, (l1 - l2).abs() / torch.maximum(l1, l2), torch.full_like(l1, math.inf))
    return dict(ratio=r_dist, vclip=v_dist, branch=b_dist, ratio_outside=(ratio < lo) | (ratio > hi), value_outside=outside)


def near_edges(d):
    """masks of the samples inside the margins (the samples a tie case put on a value-clip edge are not `near` it: they are on it)"""
    e = edge_distances(d)
    free = ~d["tie_rows"]
    return dict(ratio=e["ratio"] < RATIO_MARGIN, vclip=(e["vclip"] < VCLIP_MARGIN) & free, branch=(e["branch"] < BRANCH_MARGIN) & free)


def repair(d, rounds=200):
    """move every sample near an edge off it and look again; returns the share of samples that was moved at least once.  The two squared
    errors differ by (v - vc) (v + vc - 2 R): just outside the clip v - vc is small, and they are 1 % apart only for a return within
    some 100 |v - vc| of the value; so the returns step TOWARDS the value, and a sample far from it takes several steps."""
    idx, st = d["idx"], d["storage"]
    moved = torch.zeros(idx.numel(), dtype=torch.bool)
    for _ in range(rounds):
        n = near_edges(d)
        if not (n["ratio"] | n["vclip"] | n["branch"]).any():
            break
        st["old_logp"][idx[n["ratio"]]] += 0.05
        st["old_values"][idx[n["vclip"]]] += 0.01
        to_v = torch.sign(d["value"].float() - st["returns"][idx])
        st["returns"][idx[n["branch"]]] += 0.05 * torch.where(to_v == 0, torch.ones_like(to_v), to_v)[n["branch"]]
        moved |= n["ratio"] | n["vclip"] | n["branch"]
    return float(moved.double().mean())


def loss_inputs(c):
    """CPU tensors of one case: mean [rows, A] and value [rows] in bf16, std [A] fp32, idx int64 [rows], the fp32 storage
    (2 * rows + 7 entries: idx is a permuted subset), all from one CPU generator seeded by the case's name"""
    g = torch.Generator().manual_seed(_seed(c.name))
    rows, A = c.rows, c.A
    S = 2 * rows + 7
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    uni = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 0.5 + 0.5
    idx = torch.randperm(S, generator=g)[:rows].contiguous()
    mean, value, std = rnd(rows, A).to(torch.bfloat16), rnd(rows).to(torch.bfloat16), uni(A).float()
    st = {k: rnd(S, A).float() for k in ("actions", "old_mu")}
    st["old_sigma"] = uni(S, A).float()
    st.update({k: rnd(S).float() for k in ("old_logp", "advantages", "returns", "old_values")})
    # the new policy near the old one: ratios and value differences on both sides of their clip ranges
    st["actions"][idx] = (mean.double() + std.double() * rnd(rows, A)).float()
    st["old_mu"][idx] = (mean.double() + 0.1 * rnd(rows, A)).float()
    logp = _log_prob(st["actions"][idx].double(), mean.double(), std.double())
    st["old_logp"][idx] = (logp + 0.3 * rnd(rows)).float()
    tie_rows = torch.zeros(rows, dtype=torch.bool)
    if c.tie:
        k = min(rows, TIES)
        tie_rows[:k] = True
        value[:k] = 0
    st["old_values"][idx] = (value.double() + 0.3 * rnd(rows)).float()
    st["returns"][idx] = (value.double() + rnd(rows)).float()
    if c.tie:
        sign = torch.tensor([1.0, -1.0]).repeat(TIES)[:k]
        st["old_values"][idx[:k]] = (sign * CLIP).float()                    # v - v_old = -+clip, exactly
        R = st["returns"][idx[:k]]
        st["returns"][idx[:k]] = torch.where(R.abs() < 0.25, R + 0.5, R)     # the gradient 2 (v - R) is not a small number
    d = dict(case=c, mean=mean, value=value, std=std, idx=idx, storage=st, tie_rows=tie_rows)
    d["raw_near"] = {k: float(m.double().mean()) for k, m in near_edges(d).items()}
    d["moved"] = repair(d)
    return d


def mse_inputs(c):
    g = torch.Generator().manual_seed(_seed(c.name))
    S = 2 * c.rows + 3
    idx = torch.randperm(S, generator=g)[:c.rows].contiguous()
    target = torch.randn(S, c.npv, generator=g, dtype=torch.float64).float()
    pred = (target[idx].double() + 0.5 * torch.randn(c.rows, c.npv, generator=g, dtype=torch.float64)).to(torch.bfloat16)
    return dict(case=c, pred=pred, target=target, idx=idx)


# ------------------------------------------------------------------------------------------------------------------ models
def loss_model(d):
    """the statements of ppo.py's mini-batch step in float64; gradients by autograd of `loss`"""
    c, idx, st = d["case"], d["idx"], d["storage"]
    rows, A = c.rows, c.A
    b = {k: st[k][idx].double() for k in _STORAGE}
    mu = d["mean"].double().requires_grad_()
    value = d["value"].double().requires_grad_()
    sigma = d["std"].double().expand(rows, A).clone().requires_grad_()       # a leaf per sample: the samples' shares of d_std
    sigma_e = d["std"].double().clone().requires_grad_()                     # the entropy's sigma
    # Normal(mu, sigma): log_prob(actions).sum(-1), entropy().sum(-1)
    logp = (-((b["actions"] - mu) ** 2) / (2 * sigma ** 2) - torch.log(sigma) - math.log(math.sqrt(2 * math.pi))).sum(-1)
    logp.retain_grad()
    entropy = (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(sigma_e)).expand(rows, A).sum(-1)
    with torch.no_grad():
        kl_terms = torch.log(sigma / b["old_sigma"] + 1.e-5) + (torch.square(b["old_sigma"]) + torch.square(b["old_mu"] - mu)) / (2.0 * torch.square(sigma)) - 0.5
        kl_mean = torch.mean(torch.sum(kl_terms, axis=-1))
    ratio = torch.exp(logp - b["old_logp"])
    surrogate = -b["advantages"] * ratio
    surrogate_clipped = -b["advantages"] * torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP)
    surrogate_terms = torch.max(surrogate, surrogate_clipped)
    surrogate_loss = surrogate_terms.mean()
    if c.clipped:
        value_clipped = b["old_values"] + (value - b["old_values"]).clamp(-CLIP, CLIP)
        value_terms = torch.max((value - b["returns"]).pow(2), (value_clipped - b["returns"]).pow(2))
    else:
        value_terms = (b["returns"] - value).pow(2)
    value_loss = value_terms.mean()
    loss = surrogate_loss + VALUE_COEF * value_loss - ENTROPY_COEF * entropy.mean()
    loss.backward()
    u22 = 2.0 ** -22
    return dict(
        surrogate=float(surrogate_loss.detach()), value_loss=float(value_loss.detach()), kl=float(kl_mean),
        surrogate_abs=float(surrogate_terms.detach().abs().sum() / rows), value_loss_abs=float(value_terms.detach().abs().sum() / rows),
        kl_abs=float(kl_terms.abs().sum() / rows),
        d_std=sigma.grad.sum(0) + sigma_e.grad, d_std_abs=sigma.grad.abs().sum(0) + sigma_e.grad.abs(),
        d_mean=mu.grad, d_value=value.grad,
        # what the fp32 differences a - mu and v - R may lose, carried to the gradient
        d_mean_atol=u22 * (b["actions"].abs() + mu.detach().abs()) / d["std"].double() ** 2 * logp.grad.abs()[:, None],
        d_value_atol=u22 * (value.detach().abs() + b["returns"].abs()) * 2.0 * VALUE_COEF / rows,
        edges=edge_distances(d))


def mse_model(d):
    import torch.nn.functional as F
    c = d["case"]
    pred = d["pred"].double().requires_grad_()
    target = d["target"][d["idx"]].double()
    sel = [0] if c.selective else list(range(c.npv))
    n = c.num_train
    train = F.mse_loss(pred[:n, sel], target[:n, sel])
    test = F.mse_loss(pred[n:, sel], target[n:, sel])
    train.backward()
    return dict(train_loss=float(train.detach()), test_loss=float(test.detach()), d_pred=pred.grad,
                d_pred_atol=2.0 ** -22 * (pred.detach().abs() + target.abs()) * 2.0 / (n * len(sel)))


# ------------------------------------------------------------------------------------------------------------------ bounds
def grad_bound(ref, atol):
    """per-sample bf16 gradients: one bf16 ulp (2^-8 relative: the store's rounding is half of it, the other half is left for the fp32
    evaluation of logp and expf) plus the cancellation term"""
    return 2.0 ** -8 * ref.abs() + atol


def n_add(rows):
    """additions a sum goes through: the 64-lane butterfly, the four waves, the walk over the workgroups' rows"""
    return 6 + 4 + (rows + 255) // 256


def sum_bound(rows, abs_sum, eps_term):
    return (n_add(rows) * 2.0 ** -24 + eps_term) * abs_sum
