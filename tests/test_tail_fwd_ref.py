"""The models, bounds and case tables of tests/tail_fwd_ref.py, checked without a GPU: the bf16 rounding against torch's on every one of
the 2^16 upper halves and on the ties; one layer and the ELU-on-load against torch float64 addmm, F.elu and an explicit loop; the tables
cover what they must; the exactness condition of every exact case; the 1 % two-valued-interval condition of the ELU families; the fp32
left-to-right reference inside the bounds of every rounded case, with its mismatch share (twice that share is the kernel's cap); and
deliberately wrong evaluations (a dropped last k-step, l0 and l1 swapped, ELU on the head) outside the bounds in at least one case of
their family.  Run with -s for the figures."""
import numpy as np
import pytest
import torch

import tail_fwd_ref as T
from ppo_rollout_ref import bf16_bits, bf16_is_nan, bf16_widen


def as_torch_bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ bf16 rounding
def test_bf16_rounding_equals_torch_on_all_patterns_and_ties():
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    for low in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
        p = hi | np.uint32(low)
        x = p.view(np.float32)
        ok = ~np.isnan(x)
        got = bf16_bits(x)
        want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert (got[ok] == want[ok]).all(), hex(low)
        assert bf16_is_nan(got[~ok]).all() and bf16_is_nan(want[~ok]).all()
        if low == 0x8000:                                           # a tie goes to the even neighbour
            up = (p >> 16) + ((p >> 16) & 1)
            fin = ok & (((p >> 16) & 0x7FFF) < 0x7F80)
            assert (got[fin] == up[fin].astype(np.uint16)).all()
    exact = np.arange(1 << 16, dtype=np.uint16)
    ok = ~bf16_is_nan(exact)
    assert (bf16_bits(bf16_widen(exact[ok])) == exact[ok]).all() and (T.round_bf16(T.widen64(exact[ok])) == exact[ok]).all()


# ------------------------------------------------------------------------------------------------------------------ the two operations
def test_layer_equals_torch_float64():
    d = T.rounded_inputs(T.ROUNDED_CASES[2])[0]
    a, W, b = d["x"], d["W"][0], d["b"][0]
    ta, tW, tb = (as_torch_bf16(t).double() for t in (a, W, b))
    z = torch.addmm(tb, ta, tW.t())
    v, e = T.layer(a, W, b, elu=False)
    np.testing.assert_allclose(v, z.numpy(), rtol=1e-13, atol=1e-13)
    ve, ee = T.layer(a, W, b, elu=True)
    np.testing.assert_allclose(ve, torch.nn.functional.elu(z).numpy(), rtol=1e-13, atol=1e-13)
    assert (ee >= e).all() and (e > 0).all()
    # an explicit loop over one row: value, sum of magnitudes and the bound's formula
    r, K = 5, a.shape[1]
    for n in (0, 17, W.shape[0] - 1):
        s = float(tb[n]) + sum(float(ta[r, k]) * float(tW[n, k]) for k in range(K))
        mag = abs(float(tb[n])) + sum(abs(float(ta[r, k]) * float(tW[n, k])) for k in range(K))
        assert abs(v[r, n] - s) <= 1e-12 and abs(e[r, n] - 2 * (K + 2) * 2.0 ** -24 * mag) <= 1e-18


def test_elu_on_load_equals_torch_float64_and_a_loop():
    d = T.elu_inputs(next(c for c in T.ELU_CASES if c.npv == 3 and c.lat_cols == c.cols))
    c = d["case"]
    x, lat, wz = d["y"][:, :c.cols], d["lat"][:, :c.npv], d["wz"][:, :c.npv]
    tx, tl, tw = (as_torch_bf16(t).double() for t in (x, lat, wz))
    want = torch.nn.functional.elu(tx + tl @ tw.t())
    v, e = T.elu_on_load(x, lat, wz)
    np.testing.assert_allclose(v, want.numpy(), rtol=1e-13, atol=1e-15)
    for r, col in ((0, 0), (c.rows - 1, c.cols - 1), (c.rows // 2, 9)):
        s = float(tx[r, col]) + sum(float(tl[r, q]) * float(tw[col, q]) for q in range(c.npv))
        assert abs(v[r, col] - (s if s > 0 else np.expm1(s))) <= 1e-14
        mag = abs(float(tx[r, col])) + sum(abs(float(tl[r, q]) * float(tw[col, q])) for q in range(c.npv))
        assert e[r, col] >= c.npv * 2.0 ** -24 * mag
    v0, e0 = T.elu_on_load(x)
    np.testing.assert_allclose(v0, torch.nn.functional.elu(tx).numpy(), rtol=1e-13, atol=1e-15)
    assert (e0[bf16_widen(x) > 0] == 0).all()                       # a positive pre-activation without a latent passes unchanged


def test_elu1_bound_branches():
    u = 2.0 ** -24
    assert T.elu1_bound(np.array([1.0]), np.array([0.0]))[0] == 0.0
    t = 5e-4
    assert T.elu1_bound(np.array([-t]), np.array([0.0]))[0] == pytest.approx(t ** 3 / 6 + 2 * u * t, rel=1e-12)
    assert T.elu1_bound(np.array([-1.0]), np.array([0.0]))[0] == pytest.approx(2 * 2.0 ** -25 + u * (1 - np.exp(-1.0)), rel=1e-12)
    # undecided branches take the larger candidate
    assert T.elu1_bound(np.array([1e-9]), np.array([1e-8]))[0] > 0.0
    both = T.elu1_bound(np.array([-1e-3]), np.array([1e-6]))[0]
    assert both >= 1e-9 / 6 + 2 * u * 1e-3 and both >= 2 * u + u * 1e-3 * 0.999
    # the series really is that close to expm1 in float64, and fp32 elu1 lies inside the bound on a sweep of both branches
    x = -np.logspace(-8, 1.2, 4000)
    xb = bf16_bits(x.astype(np.float32))
    v, e = T.elu_on_load(xb[None, :])
    got = T.elu1_fp32(bf16_widen(xb)).astype(np.float64)
    assert (np.abs(got - v[0]) <= e[0]).all()


# ------------------------------------------------------------------------------------------------------------------ tables
def ksteps(k):
    return k // 32


def test_tables_cover_what_they_must():
    E = T.EXACT_CASES
    assert len({c.name for c in E}) == len(E) and 25 <= len(E) <= 35
    layers = [(n.dims[l], n.dims[l + 1]) for c in E for n in c.nets for l in range(len(n.dims) - 1)]
    assert {32, 64, 96, 128, 160, 256, 288, 512} <= {k for k, _ in layers}
    assert {1, 2, 3, 4, 5, 8, 9, 16} <= {ksteps(k) for k, _ in layers} and {1, 2, 3, 4} == {(ksteps(k) + 3) // 4 for k, _ in layers}
    assert {16, 48, 64, 80, 256, 272, 512} <= {n for _, n in layers} and {1, 3, 4, 5, 16, 17, 32} <= {n // 16 for _, n in layers}
    assert {1, 31, 32, 33, 65} == {n.rows for c in E for n in c.nets}
    assert {1, 2, 3, 4} == {len(n.dims) - 1 for c in E for n in c.nets} and {1, 2, 3} == {len(c.nets) for c in E}
    for k, n in layers:
        assert k % 32 == 0 and n % 16 == 0 and k <= 512 and n <= 512
    multi = [c for c in E if len(c.nets) > 1]
    key = lambda n: (n.rows, len(n.dims))
    assert any(key(c.nets[0]) == min(map(key, c.nets)) and len({key(n) for n in c.nets}) > 1 for c in multi)        # the shortest net first
    assert any(key(c.nets[-1]) == min(map(key, c.nets)) and len({key(n) for n in c.nets}) > 1 for c in multi)       # ... and last
    assert any(len({n.rows for n in c.nets}) > 1 and len({len(n.dims) for n in c.nets}) > 1 for c in multi)
    assert any(n.in_ld > n.dims[0] and n.in_off > 0 for c in E for n in c.nets) and all(n.in_off % 8 == 0 for c in E for n in c.nets)
    assert {0, 3, 8} <= {n.out_pad for c in E for n in c.nets}
    assert any(any(n.elu) for c in E for n in c.nets)
    R = T.ROUNDED_CASES
    assert {(512, 256, 128, 64), (256, 128, 64)} == {c.dims for c in R} and {33, 65} == {c.rows for c in R} and len(R) == 4
    for c in R:
        assert all(d["net"].elu == (1,) * (len(c.dims) - 2) + (0,) for d in T.rounded_inputs(c))
    L = T.ELU_CASES
    assert {1, 63, 64, 65, 130} == {c.rows for c in L} and {8, 120, 128, 136} == {c.cols for c in L} and all(c.ld > c.cols for c in L)
    assert {0, 1, 2, 3, 5} == {c.npv for c in L}
    withlat = [c for c in L if c.npv]
    assert any(c.lat_cols == 0 for c in withlat) and any(c.lat_cols == 8 for c in withlat) and any(c.lat_cols == c.cols for c in withlat)
    assert any(c.lat_cols == c.cols // 16 * 8 and 8 < c.lat_cols < c.cols for c in withlat)
    paths = {(n.npv, T.load_path(n)) for c in T.LOAD_CASES for n in c.nets}
    assert {(1, "general"), (2, "lat2"), (2, "general"), (3, "general"), (5, "general"), (0, "none")} == paths
    assert {1, 63, 64, 65, 130} <= {n.rows for c in T.LOAD_CASES for n in c.nets}
    general2 = [n for c in T.LOAD_CASES for n in c.nets if n.npv == 2 and T.load_path(n) == "general"]
    assert any(n.lat_ld % 2 for n in general2) and any(n.wz_ld % 2 for n in general2) and any(n.lat_off % 2 for n in general2) and any(n.wz_off % 2 for n in general2)
    assert any({T.load_path(n) for n in c.nets} == {"lat2", "none"} for c in T.LOAD_CASES)
    for c in T.LOAD_CASES:
        for n in c.nets:
            assert n.k % 32 == 0 and n.k <= 512 and (n.npv == 0 or (n.lat_ld >= n.npv and n.wz_ld >= n.npv))


# ------------------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("c", T.EXACT_CASES, ids=lambda c: c.name)
def test_exact_case_satisfies_the_exactness_condition(c):
    """exact_model asserts, per layer: operands on the grid, sum |term| / grid < 2^24, ELU layers with pre-activations >= 0, the output
    on the grid.  Here also: the float64 evaluation of the same data agrees bit for bit, and the outputs are not trivial"""
    worst = 0.0
    for d in T.exact_inputs(c):
        n = d["net"]
        outs = T.exact_model(d)
        a, grid = d["x"][:, n.in_off:n.in_off + n.dims[0]], T.IN_GRID
        for l, out in enumerate(outs):
            _, grid_out, used = T.exact_layer(a, d["W"][l], d["b"][l], n.elu[l], grid)
            worst = max(worst, used)
            v, _ = T.layer(a, d["W"][l], d["b"][l], n.elu[l])
            assert (T.round_bf16(v) == out).all()
            vals = bf16_widen(out)
            assert len(np.unique(vals)) > min(8, vals.size // 2)
            if not n.elu[l]:
                assert (vals < 0).any() or vals.size < 32
            a, grid = out, grid_out
    print(f"\ntail_fwd_ref exact [{c.name}]: largest sum |term| / grid = {worst:.4f} of 2^24", end="")
    assert worst < 1.0


# ------------------------------------------------------------------------------------------------------------------ rounded cases
@pytest.mark.parametrize("c", T.ROUNDED_CASES, ids=lambda c: c.name)
def test_fp32_left_to_right_lies_inside_the_bounds(c):
    nets = T.rounded_inputs(c)
    outside, share, worst = T.shares(nets, [T.rounded_fp32(d) for d in nets])
    print(f"\ntail_fwd_ref rounded [{c.name}]: fp32 left-to-right outside={outside} ratio={worst:.5f} mismatch share={share:.6f} "
          f"({round(share * T.elements(nets))} of {T.elements(nets)}; the kernel's cap: {2 * share:.6f})", end="")
    assert outside == 0 and share == T.reference_share(c)
    assert round(share * T.elements(nets)) >= T.ROUNDED_MIN_REFERENCE_COUNT, "too few reference mismatches for a cap: take the next seed suffix"


# ------------------------------------------------------------------------------------------------------------------ ELU families
@pytest.mark.parametrize("c", T.ELU_CASES, ids=lambda c: c.name)
def test_elu_case_intervals_and_fp32(c):
    d = T.elu_inputs(c)
    v, e = T.elu_model(d)
    share = T.two_valued(v, e)
    lat_on = c.npv and c.lat_cols
    got = T.elu_fp32(d["y"][:, :c.cols])
    if lat_on:
        got[:, :c.lat_cols] = T.elu_fp32(d["y"][:, :c.lat_cols], d["lat"][:, :c.npv], d["wz"][:c.lat_cols, :c.npv])
    outside, mismatch = T.compare(got, v, e)
    print(f"\ntail_fwd_ref elu [{c.name}]: two-valued share={share:.5f}  fp32 numpy outside={int(outside.sum())} mismatch={mismatch.mean():.5f}", end="")
    assert share <= 0.01 and not outside.any()
    x = bf16_widen(d["y"][:, :c.cols])
    assert ((x > -1e-3) & (x < 0)).any() and (x < -1.0).any() and (x > 0).any() and (x == 0).any() or x.size < 64


@pytest.mark.parametrize("c", T.LOAD_CASES, ids=lambda c: c.name)
def test_load_case_intervals_and_fp32(c):
    for d in T.load_inputs(c):
        n = d["net"]
        v, e = T.load_model(d)
        share = T.two_valued(v, e)
        got = T.elu_fp32(d["x"][:, :n.k], *((d["lat"][:, :n.npv], d["wz"][:, :n.npv]) if n.npv else ()))
        outside, mismatch = T.compare(got, v, e)
        print(f"\ntail_fwd_ref load [{c.name}] {T.load_path(n)}: two-valued share={share:.5f}  fp32 numpy outside={int(outside.sum())} "
              f"mismatch={mismatch.mean():.5f}", end="")
        assert share <= 0.01 and not outside.any()
        # the identity layer hands the activated input through bit for bit, in the model too
        v1, _ = T.layer(got, d["W"][0], d["b"][0], elu=False)
        assert (T.round_bf16(v1) == got).all()


# ------------------------------------------------------------------------------------------------------------------ wrong evaluations
@pytest.mark.parametrize("variant", ["drop_last_kstep", "elu_on_head"])
def test_wrong_exact_evaluation_is_rejected(variant):
    failing = []
    for c in T.EXACT_CASES:
        for d in T.exact_inputs(c):
            if any((w != r).any() for w, r in zip(T.exact_model(d, variant), T.exact_model(d))):
                failing.append(c.name)
                break
    assert failing
    if variant == "drop_last_kstep":
        assert len(failing) == len(T.EXACT_CASES)
    else:                                                           # every case whose head has no ELU of its own
        assert set(failing) == {c.name for c in T.EXACT_CASES if any(not n.elu[-1] for n in c.nets)}


@pytest.mark.parametrize("variant", ["drop_last_kstep", "elu_on_head"])
def test_wrong_rounded_evaluation_is_rejected(variant):
    for c in T.ROUNDED_CASES:
        nets = T.rounded_inputs(c)
        outside, _, _ = T.shares(nets, [T.rounded_fp32(d, variant) for d in nets])
        assert outside > 0, c.name


def test_swapped_latent_columns_are_rejected():
    swap = lambda lat: lat[:, [1, 0] + list(range(2, lat.shape[1]))]
    failing = []
    for c in T.ELU_CASES:
        if c.npv >= 2 and c.lat_cols:
            d = T.elu_inputs(c)
            got = T.elu_fp32(d["y"][:, :c.lat_cols], swap(d["lat"][:, :c.npv]), d["wz"][:c.lat_cols, :c.npv])
            v, e = T.elu_model(d)
            failing.append(bool(T.compare(got, v[:, :c.lat_cols], e[:, :c.lat_cols])[0].any()))
    assert failing and all(failing)
    failing = []
    for c in T.LOAD_CASES:
        for d in T.load_inputs(c):
            n = d["net"]
            if n.npv >= 2:
                got = T.elu_fp32(d["x"][:, :n.k], swap(d["lat"][:, :n.npv]), d["wz"][:, :n.npv])
                failing.append(bool(T.compare(got, *T.load_model(d))[0].any()))
    assert failing and all(failing)


def test_a_nan_is_outside_every_interval():
    v, e = np.array([[1.0, -0.5]]), np.array([[1.0, 1.0]])
    got = T.round_bf16(v)
    assert not T.compare(got, v, e)[0].any()
    got[0, 0] = 0x7FC0
    outside, mismatch = T.compare(got, v, e)
    assert outside[0, 0] and mismatch[0, 0] and not outside[0, 1] and T.ratio_to_bound(got, v, e) == float("inf")
