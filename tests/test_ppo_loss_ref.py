"""The input recipe and the float64 model of tests/ppo_loss_ref.py, checked without a GPU: after the repair no sample of any case of the
GPU tables lies inside the margins around a decision edge, both sides of both clips are well populated, the constructed ties sit exactly
on their edge, and autograd's per-sample gradients are the closed form that csrc/go1ppo.hip quotes above loss_sample, tie rule included."""
import pytest
import torch

import ppo_loss_ref as P


_made = {}


def made(c):
    if c.name not in _made:
        _made[c.name] = P.loss_inputs(c)
    return _made[c.name]


@pytest.fixture(params=P.LOSS_CASES, ids=lambda c: c.name)
def inputs(request):
    return made(request.param)


def test_tables_cover_what_they_must():
    L, M = P.LOSS_CASES, P.MSE_CASES
    assert len(L) <= 40 and len(M) <= 40 and len({c.name for c in L}) == len(L) and len({c.name for c in M}) == len(M)
    assert {1, 64, 65, 256, 257, 1031, 8259} <= {c.rows for c in L}
    assert {1, 4, 5, 8, 12, 16, 32} <= {c.A for c in L} and {0, 1} == {c.clipped for c in L} and {64, 36, 34} <= {c.head_ld for c in L}
    assert any(c.null_old_values and not c.clipped for c in L) and not any(c.null_old_values and c.clipped for c in L)
    for off in (dict(actions=1), dict(old_sigma=1), dict(mean=2), dict(d_mean=2)):
        assert any(c.A == 12 and c.off == off for c in L), off
    assert {"vector", "scalar", "vector loads, scalar stores", "wide heads"} == {P.loss_family(c) for c in L}
    assert P.loss_family(next(c for c in L if c.off == dict(d_mean=2) and c.A == 12)) == "vector loads, scalar stores"
    assert {1, 2, 6, 7, 9, 13, 64} <= {c.npv for c in M} and {0, 1} == {c.selective for c in M} and {64, 72} == {c.pred_ld for c in M}
    assert {(2, 1), (257, 1), (257, 256), (257, 128), (1000, 800)} <= {(c.rows, c.num_train) for c in M}
    assert len({P.mse_family(c) for c in M}) == 3


def test_no_sample_is_left_near_an_edge(inputs):
    near = P.near_edges(inputs)
    for name, mask in near.items():
        assert int(mask.sum()) == 0, (name, int(mask.sum()))
    # the raw recipe leaves few samples to move (a recipe that had to move many would no longer be the distribution it describes)
    assert inputs["moved"] <= 0.1 or inputs["case"].rows < 64, inputs["moved"]


def test_every_case_has_gradients_to_compare(inputs):
    m = P.loss_model(inputs)
    assert float(m["d_mean"].abs().max()) > 0 and float(m["d_value"].abs().max()) > 0
    assert bool((m["d_mean_atol"] >= 0).all()) and bool((m["d_value_atol"] >= 0).all()) and bool((m["d_std_abs"] > 0).all())


@pytest.mark.parametrize("c", [c for c in P.LOSS_CASES if c.rows >= 64], ids=lambda c: c.name)
def test_both_sides_of_both_clips_are_populated(c):
    e = P.edge_distances(made(c))
    for name in ("ratio_outside", "value_outside"):
        share = float(e[name].double().mean())
        assert 0.2 <= share <= 0.8, (name, share)


def test_ties_sit_exactly_on_the_value_clip():
    for c in (c for c in P.LOSS_CASES if c.tie):
        d = P.loss_inputs(c)
        k = int(d["tie_rows"].sum())
        assert k == min(c.rows, P.TIES) and c.clipped
        v, vo = d["value"][:k], d["storage"]["old_values"][d["idx"][:k]]
        for dlt in (v.float() - vo, v.double() - vo.double()):               # as the kernel forms it, and as the model does
            assert torch.equal(dlt.abs().double(), torch.full((k,), P.CLIP, dtype=torch.float64))
        assert bool((v.float() - vo > 0).any()) and bool((v.float() - vo < 0).any())      # both edges


def test_autograd_equals_the_quoted_closed_form():
    """d surrogate / d logp = -adv ratio / M where the un-clamped branch is active (inside the clip range both branches coincide and
    torch.max splits the gradient onto two identical paths), else 0; the value loss with the same tie rule"""
    c = next(c for c in P.LOSS_CASES if c.name == "tie-A12")
    d = P.loss_inputs(c)
    m = P.loss_model(d)
    idx, st = d["idx"], d["storage"]
    b = {k: st[k][idx].double() for k in ("actions", "old_logp", "advantages", "returns", "old_values")}
    mu, v, sg = d["mean"].double(), d["value"].double(), d["std"].double()
    z = (b["actions"] - mu) / sg
    ratio = torch.exp((-0.5 * z * z - torch.log(sg) - 0.9189385332046727).sum(-1) - b["old_logp"])
    lo, hi = 1.0 - P.CLIP, 1.0 + P.CLIP
    s1, s2 = -b["advantages"] * ratio, -b["advantages"] * ratio.clamp(lo, hi)
    active = ((ratio >= lo) & (ratio <= hi)) | (s1 > s2)
    dlogp = torch.where(active, -b["advantages"] * ratio / c.rows, torch.zeros_like(ratio))
    torch.testing.assert_close(m["d_mean"], dlogp[:, None] * z / sg, rtol=1e-12, atol=1e-18)
    dlt = v - b["old_values"]
    l1, l2 = (v - b["returns"]) ** 2, (b["old_values"] + dlt.clamp(-P.CLIP, P.CLIP) - b["returns"]) ** 2
    v_active = ((dlt >= -P.CLIP) & (dlt <= P.CLIP)) | (l1 > l2)
    want = torch.where(v_active, P.VALUE_COEF * 2.0 * (v - b["returns"]) / c.rows, torch.zeros_like(v))
    torch.testing.assert_close(m["d_value"], want, rtol=1e-12, atol=1e-18)
    # the case does exercise all of it: ties on the edge with a gradient that `>` for `>=` would lose, and both branches outside
    on_edge = dlt.abs() == P.CLIP
    assert int(on_edge.sum()) == P.TIES and bool((want[on_edge].abs() > 1e-4).all())
    assert bool((~v_active).any()) and bool((v_active & (dlt.abs() > P.CLIP)).any()) and bool((~active).any())
    # d_std: the samples' shares and the entropy's
    want_std = (dlogp[:, None] * (z * z - 1.0) / sg).sum(0) - P.ENTROPY_COEF / sg
    torch.testing.assert_close(m["d_std"], want_std, rtol=1e-10, atol=1e-16)


def test_mse_model_zeroes_what_carries_no_gradient():
    for c in P.MSE_CASES:
        m = P.mse_model(P.mse_inputs(c))
        g = m["d_pred"]
        assert not g[c.num_train:].any() and bool(g[:c.num_train, 0].any())
        if c.selective and c.npv > 1:
            assert not g[:, 1:].any()
        assert m["train_loss"] > 0 and m["test_loss"] > 0
