"""The float64 models, bounds and case tables of tests/ppo_rollout_ref.py, checked without a GPU: the tables cover what they must; the
kernels' statements evaluated in fp32 numpy (a rounding after every operation) lie inside the models' bounds on every case; deliberately
wrong fp32 variants, sent through the same comparators, are rejected; and the models equal RolloutStorage.compute_returns and
gaussian_log_prob run in float64 on the CPU.  Run with -s for the worst error-to-bound ratio of every family."""
import numpy as np
import pytest
import torch

import ppo_rollout_ref as R


def worst_by_check(all_checks):
    out = {}
    for checks in all_checks:
        for k, (e, b) in checks.items():
            k = "X" if k[0] == "X" and k[1:].isdigit() else k
            out[k] = max(out.get(k, 0.0), R.ratio(e, b))
    return out


def report(family, ratios):
    print(f"\nppo_rollout_ref fp32 numpy [{family}]: " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(ratios.items())), end="")
    assert all(v <= 1.0 for v in ratios.values()), (family, ratios)


def rejected_somewhere(cases, inputs, wrong, compare):
    return any(not R.passes(compare(d, wrong(d))) for d in map(inputs, cases))


# ------------------------------------------------------------------------------------------------------------------ tables
def test_tables_cover_what_they_must():
    for table in (R.ACT_CASES, R.STORE_CASES, R.GAE_CASES, R.NORM_CASES, R.RING_CASES):
        assert len({c.name for c in table}) == len(table) <= 16
    A = R.ACT_CASES
    assert {1, 63, 64, 65, 257} == {c.rows for c in A} and {1, 5, 12, 32} == {c.A for c in A} and {36, 64} <= {c.head_ld for c in A}
    assert any(c.head_ld == c.A for c in A) and all(c.head_ld >= c.A for c in A) and {True, False} == {c.shared for c in A}
    logs = np.concatenate([np.log(R.act_inputs(c)["std"].astype(np.float64)) for c in A])
    assert logs.min() < -1.0 and logs.max() > 0.5                              # log sigma of both signs
    for c in A:
        d = R.act_inputs(c)
        assert 0.05 <= d["std"].min() and d["std"].max() <= 2.0 and float(np.abs(R.bf16_widen(d["mean"])).max()) == 8.0
        if c.rows * c.A > 1:
            sn = np.abs(d["std"].astype(np.float64) * d["noise"])
            assert (d["noise"] == 0).any() and (np.abs(sn[sn > 0] - 1e-3) < 1e-9).any()
    S = R.STORE_CASES
    assert {1, 255, 256, 257, 1000} == {c.n for c in S} and {(a, b) for a in (True, False) for b in (True, False)} == {(c.time_outs, c.env_bins) for c in S}
    assert {0.0, 0.05, 1.0} == {c.share for c in S if c.time_outs}
    for c in S:
        d = R.store_inputs(c)
        if c.time_outs:
            share = d["time_outs"].mean()
            assert share == c.share if c.share in (0.0, 1.0) else 0 < share < 0.15
        if c.env_bins and c.n >= 5:
            assert set(R.SPECIAL_BINS) <= set(d["env_bins"].tolist())
    assert {0, -1, 16777216, 16777217, 2147483647} == set(R.SPECIAL_BINS)
    G = R.GAE_CASES
    assert {(1, 1), (1, 64), (2, 63), (7, 65), (7, 256), (24, 257), (3, 1000), (24, 1025)} == {(c.T, c.N) for c in G}
    assert set(R.GAE_DONES) == {c.dones for c in G} and sum(c.scale == 100.0 for c in G) == 1
    assert {(R.GAMMA, R.LAM), (1.0, 1.0)} == {(c.gamma, c.lam) for c in G}
    assert R.GAMMA == float(np.float32(0.99)) != 0.99 and R.LAM == float(np.float32(0.95)) and R.EPS == float(np.float32(1e-8))
    for c in G:
        dn = R.gae_inputs(c)["dones"]
        want = dict(none=dn.sum() == 0, all=dn.all(), last=dn[-1].all() and dn.sum() == c.N, first=dn[0].all() and dn.sum() == c.N,
                    random=0 < dn.sum() and (dn.mean() < 0.2 or dn.size < 64))
        assert want[c.dones], c.name
    assert tuple(R.gae_workgroups(n) for n in R.TICKET_N) == (1, 2, 4, 1, 5) and R.TICKET_N == (1, 257, 1000, 64, 1025)
    Nm = R.NORM_CASES
    assert {2, 255, 257, 1000} == {c.n for c in Nm} and {"plain", "two-ranks", "constant", "negative-variance"} == {c.kind for c in Nm}
    for c in Nm:
        d = R.norm_inputs(c)
        mean, var = R.norm_moments(d["stats"])
        if c.kind in ("plain", "two-ranks"):
            assert var > 0 and abs(mean) <= 1000.0 * np.sqrt(var)
        assert d["stats"][2] == (2 * c.n if c.kind == "two-ranks" else c.n)
        if c.kind == "constant":
            assert var == 0.0 and (d["adv"] == np.float32(1.5)).all()
        if c.kind == "negative-variance":
            assert -1e-6 < var < 0.0 and np.isfinite(R.norm_model(d)[0]).all() and np.abs(R.norm_model(d)[0]).max() > 100.0
    Rg = R.RING_CASES
    assert {1, 3, 4, 5, 37} == {c.N for c in Rg} and {1, 2, 5, 6, 7, 12, 13} == {c.H for c in Rg} and {2, 70, 130} == {c.no for c in Rg}
    assert {0, 1, 2, 65} == {c.npv for c in Rg} and {1, 3} == {c.T for c in Rg}
    pads = {c.Kp - R.ring_min_kp(c.H, c.no, c.npv) for c in Rg}
    assert 0 in pads and max(pads) > 2 * 128 and all(c.Kp % 2 == 0 for c in Rg)
    assert any(c.no > 128 for c in Rg) and any(c.N % 4 for c in Rg)
    for c in Rg + [R.RING_PATTERN_CASE, R.RING_WRAPPER_CASE]:
        idx = R.ring_gather_idx(c)
        assert (np.diff(idx) <= 0).all() and (np.diff(idx) == 0).any() and idx.max() == c.T * c.N - 1 and idx.min() == 0
    assert R.RING_WRAPPER_CASE.Kp % 8 == 0 and R.RING_WRAPPER_CASE.Kp - 8 < R.ring_min_kp(7, 70, 2)


def test_rounding_patterns_hold_what_the_conversion_can_get_wrong():
    p = R.rounding_patterns()
    low, e = p & 0xFFFF, (p >> 23) & 0xFF
    assert {0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF} <= set(low.tolist())
    assert ((e == 0) <= ((p & 0x7FFFFFFF) == 0)).all()                          # no subnormals
    for special in (0x0, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x7F7F8000, 0x00800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF):
        assert special in p
    x = p.view(np.float32)
    got = R.bf16_bits(x)
    # ties go to the even neighbour, whatever is above a tie goes up, the largest finite values round to infinity, NaNs stay NaNs
    tie = low == 0x8000
    up = (p >> 16) + ((p >> 16) & 1)
    ok = ~np.isnan(x)
    assert (got[tie & ok] == up[tie & ok]).all() and (got[(low > 0x8000) & ok] == ((p >> 16) + 1)[(low > 0x8000) & ok]).all()
    assert (got[(low < 0x8000) & ok] == (p >> 16)[(low < 0x8000) & ok]).all()
    assert R.bf16_bits(np.array([0x7F7F8000, 0x7F7FFFFF], np.uint32).view(np.float32)).tolist() == [0x7F80, 0x7F80]
    assert R.bf16_is_nan(got[~ok]).all() and not R.bf16_is_nan(got[ok]).any()
    # an independent conversion: torch's on the CPU
    t = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (t[ok] == got[ok]).all() and R.bf16_is_nan(t[~ok]).all()
    assert (R.bf16_bits(x, truncate=True)[ok] != got[ok]).any()
    assert (R.bf16_widen(got[ok]).view(np.uint32) == got[ok].astype(np.uint32) << 16).all()


# ------------------------------------------------------------------------------------------------------------------ fp32 numpy agreement
def test_fp32_act_lies_inside_the_bounds():
    report("act", worst_by_check(R.act_compare(d, R.act_fp32(d)) for d in map(R.act_inputs, R.ACT_CASES)))


def test_fp32_store_step_lies_inside_the_bounds():
    report("store_step", worst_by_check(R.store_compare(d, R.store_fp32(d)) for d in map(R.store_inputs, R.STORE_CASES)))
    for c in R.STORE_CASES:                                                     # the models' int32 -> fp32 conversion rounds to even
        if c.env_bins and c.n >= 5:
            d = R.store_inputs(c)
            assert R.store_fp32(d)["env_bins_out"][:5].tolist() == [16777216.0, 2147483648.0, -1.0, 0.0, 16777216.0]


def test_fp32_gae_lies_inside_the_bounds():
    all_checks = []
    for d in map(R.gae_inputs, R.GAE_CASES):
        c, got = d["case"], R.gae_fp32(d)
        checks = R.gae_compare(d, got)
        start = R.gae_stats_start(d)
        a = got["advantages"].astype(np.float64)
        checks["stats"] = R.gae_stats_check(got["advantages"], start, start + np.array([a.sum(), (a * a).sum()]), c.T, c.N)
        all_checks.append(checks)
    report("gae", worst_by_check(all_checks))


def test_fp32_normalize_lies_inside_the_bounds():
    ds = list(map(R.norm_inputs, R.NORM_CASES))
    report("normalize", worst_by_check(R.norm_compare(d, R.norm_fp32(d)) for d in ds))
    for d in ds:
        assert np.isfinite(R.norm_fp32(d)).all()


def torch_ring(d):
    """the ring statements with torch's CPU bf16 conversion: ring, per-step rows, gathered rows, as bf16 bit patterns"""
    c = d["case"]
    u16 = lambda t: t.contiguous().view(torch.int16).numpy().view(np.uint16)
    ring = torch.from_numpy(d["stream"].copy()).to(torch.bfloat16)
    priv = torch.from_numpy(d["priv"].copy()).to(torch.bfloat16)

    def row(s, n):
        x = torch.zeros(c.Kp, dtype=torch.bfloat16)
        x[:c.H * c.no] = ring[s:s + c.H, n].reshape(-1)
        x[c.H * c.no] = 1.0
        x[c.H * c.no + 1:c.H * c.no + 1 + c.npv] = priv[s, n]
        return x
    idx = R.ring_gather_idx(c)
    return dict(ring=u16(ring), X=[u16(torch.stack([row(s, n) for n in range(c.N)])) for s in range(c.T)],
                gathered=u16(torch.stack([row(int(f) // c.N, int(f) % c.N) for f in idx])))


def test_torch_ring_equals_the_integer_model():
    ds = [R.ring_inputs(c) for c in R.RING_CASES] + [R.ring_inputs(R.RING_PATTERN_CASE, patterns=True)]
    assert np.isnan(ds[-1]["stream"]).any() and np.isnan(ds[-1]["priv"]).any() and np.isinf(ds[-1]["stream"]).any()
    assert not any(np.isnan(d["stream"]).any() for d in ds[:-1])
    report("ring", worst_by_check(R.ring_compare(d, torch_ring(d)) for d in ds))
    for d in ds:                                                                # the step-0 windows are the stream's first H entries
        c = d["case"]
        assert d["ld_hist"] > c.H * c.no
        assert R.passes(dict(h=R.bit_diff(d["hist"][:, :c.H * c.no].reshape(c.N, c.H, c.no), d["stream"][:c.H].transpose(1, 0, 2))))


# ------------------------------------------------------------------------------------------------------------------ wrong variants
@pytest.mark.parametrize("variant", ["no_mask_value", "no_mask_advantage", "no_lambda", "bootstrap_same_step"])
def test_wrong_gae_is_rejected(variant):
    assert rejected_somewhere(R.GAE_CASES, R.gae_inputs, lambda d: R.gae_fp32(d, variant), R.gae_compare)
    if variant.startswith("no_mask"):
        # not on one case only: on every case with a done flag that the mask acts on (the advantage behind the last step is 0, so
        # its mask acts from the step before on), and on no other
        for c in R.GAE_CASES:
            d = R.gae_inputs(c)
            acts = bool(d["dones"].any()) if variant == "no_mask_value" else bool(d["dones"][:-1].any())
            assert R.passes(R.gae_compare(d, R.gae_fp32(d, variant))) != acts, c.name


@pytest.mark.parametrize("variant", ["no_constant", "log_sigma_squared"])
def test_wrong_act_is_rejected(variant):
    assert rejected_somewhere(R.ACT_CASES, R.act_inputs, lambda d: R.act_fp32(d, variant), R.act_compare)


@pytest.mark.parametrize("variant", ["biased", "eps_inside_sqrt"])
def test_wrong_normalize_is_rejected(variant):
    assert rejected_somewhere(R.NORM_CASES, R.norm_inputs, lambda d: R.norm_fp32(d, variant), R.norm_compare)


def test_wrong_store_step_is_rejected():
    assert rejected_somewhere(R.STORE_CASES, R.store_inputs, lambda d: R.store_fp32(d, "bootstrap_all"), R.store_compare)


@pytest.mark.parametrize("variant", ["truncate", "bias_swapped", "newest_first"])
def test_wrong_ring_is_rejected(variant):
    def wrong(d):
        m = R.ring_model(d, variant)
        return dict(ring=m["ring"], X=m["X"], gathered=m["gather"](R.ring_gather_idx(d["case"])))
    assert rejected_somewhere(R.RING_CASES, R.ring_inputs, wrong, R.ring_compare)
    d = R.ring_inputs(R.RING_PATTERN_CASE, patterns=True)
    assert not R.passes(R.ring_compare(d, wrong(d)))


def test_a_nan_output_is_outside_every_bound():
    d = R.gae_inputs(R.GAE_CASES[0])
    got = R.gae_fp32(d)
    got["returns"][0, 0] = np.nan
    assert not R.passes(R.gae_compare(d, got)) and R.ratio([0.0], [0.0]) == 0.0 and R.ratio([1e-30], [0.0]) == np.inf


# ------------------------------------------------------------------------------------------------------------------ model == reference
def test_gae_and_normalize_models_equal_compute_returns_in_float64():
    from go1_gym_learn.ppo_cse.rollout_storage import RolloutStorage
    # compute_returns forms alive * gamma * lam on the fp32 `alive`, so in fp32 whatever the storage's type: gamma = 63/64 and
    # lam = 15/16, whose product is exact there, leave the whole scan to float64
    c = next(c for c in R.GAE_CASES if c.name == "T24-N257-random")._replace(gamma=0.984375, lam=0.9375)
    d = R.gae_inputs(c)
    st = RolloutStorage(c.N, c.T, [4], [2], [8], [3])
    for name in ("rewards", "values", "returns", "advantages"):
        setattr(st, name, getattr(st, name).double())
    st.rewards.copy_(torch.from_numpy(d["rewards"]).unsqueeze(-1))
    st.values.copy_(torch.from_numpy(d["values"]).unsqueeze(-1))
    st.dones.copy_(torch.from_numpy(d["dones"]).unsqueeze(-1))
    st.compute_returns(torch.from_numpy(d["last_values"]).double().unsqueeze(-1), c.gamma, c.lam)
    m = R.gae_model(d)
    np.testing.assert_allclose(st.returns.squeeze(-1).numpy(), m["returns"], rtol=1e-12, atol=1e-13)
    a = m["advantages"].ravel()
    nd = dict(case=R.NormCase("from-gae", a.size, "plain", 0.0, 1.0), adv=a, stats=np.array([a.sum(), (a * a).sum(), float(a.size)]))
    np.testing.assert_allclose(st.advantages.squeeze(-1).numpy().ravel(), R.norm_model(nd)[0], rtol=1e-9, atol=1e-11)
    assert int(d["dones"].sum()) > 100


def test_act_model_equals_gaussian_log_prob_in_float64():
    from go1_gym_learn.ppo_cse.ppo import gaussian_log_prob
    c = next(c for c in R.ACT_CASES if c.name == "rows257-A12-ld36")
    d = R.act_inputs(c)
    m = R.act_model(d)
    a = m["actions"].astype(np.float32)
    want = gaussian_log_prob(torch.from_numpy(a).double(), torch.from_numpy(m["mu"]).double(), torch.from_numpy(d["std"]).double())
    np.testing.assert_allclose(R.act_logp(d, a)[0], want.numpy(), rtol=1e-12, atol=1e-12)
    # the sampled action itself: mean + std * noise
    np.testing.assert_allclose(m["actions"], (torch.from_numpy(m["mu"]).double() + torch.from_numpy(d["std"]).double() * torch.from_numpy(d["noise"]).double()).numpy(), rtol=0, atol=0)
