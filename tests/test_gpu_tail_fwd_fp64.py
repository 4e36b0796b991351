"""go1ppo_tail_fwd (csrc/go1ppo.hip, tail_fwd_kernel<32>: the policy's inference forward at up to 2048 rows), its ELU-on-load path and
go1ppo_elu_fwd against the float64 / integer models of tests/tail_fwd_ref.py, over the tables of cases that module holds.

Buffer discipline as in test_gpu_ppo_loss_fp64.py: every buffer sits inside canaries (7), inputs, weights, biases, latents are compared
with their copies after the launch, every case is launched twice on fresh outputs and the two results are bit for bit the same, and the
columns >= n_out of an output and everything around it keep their canary.  The bounds are derived in tail_fwd_ref.py, none is taken from
what the kernels give:
  exact cases    bit for bit: RNE_bf16 of the exact pre-activation (every partial sum is exact in fp32 in any order);
  rounded cases  RNE_bf16(v - e) <= got <= RNE_bf16(v + e), e = 2 (K + 2) 2^-24 (sum |a w| + |b|) (+ the elu1 bound), each layer from
                 the kernel's own stored output of the layer before; and the share of got != RNE_bf16(v) at most twice the share of
                 the fp32 left-to-right reference on the same case.  Measured on an MI355X (profiles/tail_fwd_fp64.txt): the kernel
                 differs from RNE_bf16(v) on 4, 8, 1 and 5 elements of the four cases where the reference differs on 5, 5, 4 and 5;
  ELU on load    the interval with e = npv 2^-24 (|x| + sum |l w|) + the elu1 bound.
Bit-for-bit relations: null intermediates leave the same head; tail_fwd(elu_in = 1, latent) on pre-activations equals go1ppo_elu_fwd on a
copy followed by tail_fwd(elu_in = 0) on every stored output, on the lat2 dword path and on the general path, and leaves the
pre-activations as they were; an inference FusedNet at 37 rows gives the mean, value and latent of the direct C calls on its buffers.
Every launch is one the library accepts.  Each test prints its largest error-to-bound ratio and mismatch share (run with -s)."""
import ctypes

import numpy as np
import pytest
import torch

import tail_fwd_ref as T
from test_gpu_ppo_loss_fp64 import RATIOS, Mat, Vec, note
from test_gpu_ppo_tail_fused import PAD, stream

pytestmark = pytest.mark.gpu

FAMILIES = ("tail exact", "tail rounded", "tail null intermediates", "tail elu_in", "elu_fwd", "tail engine")


@pytest.fixture(scope="module")
def lib():
    from go1_gym_learn.ppo_cse import fused
    yield fused.load_library()
    for fam in FAMILIES:
        if fam in RATIOS:
            print(f"\ntail_fwd_fp64 family [{fam}]: " + "  ".join(f"{k}={v:.3f}" for k, v in sorted(RATIOS[fam].items())), end="")
    print()


def bf(bits):
    """bf16 bit patterns (numpy uint16) -> CPU bf16 tensor of the same bits"""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def host(x):
    """bf16 tensor -> its bit patterns (numpy uint16)"""
    return x.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def mat(bits, off=0):
    """a matrix of bf16 bit patterns, every column given, inside canaries"""
    assert PAD % 8 == 0
    return Mat(bits.shape[0], bits.shape[1], bf(bits), off=off)


def spec(d, elu_in=0):
    """one net of a launch: exact and rounded nets (tail_fwd_ref.Net) and ELU-on-load nets (LoadNet: identity, then a random layer)"""
    n = d["net"]
    if isinstance(n, T.LoadNet):
        s = dict(rows=n.rows, dims=(n.k, n.k, 48), elu=(0, 0), in_off=0, out_pad=0, npv=n.npv, lat_ld=n.lat_ld, wz_ld=n.wz_ld,
                 lat=mat(d["lat"], n.lat_off) if n.npv else None, wz=mat(d["wz"], n.wz_off) if n.npv else None)
    else:
        s = dict(rows=n.rows, dims=n.dims, elu=n.elu, in_off=n.in_off, out_pad=n.out_pad, npv=0, lat_ld=0, wz_ld=0, lat=None, wz=None)
    s.update(elu_in=elu_in, x=mat(d["x"]), W=[Vec(bf(w)) for w in d["W"]], b=[Vec(bf(b)) for b in d["b"]])
    return s


class Launch:
    """the device buffers of one go1ppo_tail_fwd launch; `run` launches on fresh outputs and checks what a launch may not touch"""

    def __init__(self, specs):
        self.specs = specs

    def inputs(self):
        for i, s in enumerate(self.specs):
            yield f"net{i}.x", s["x"]
            for l, (w, b) in enumerate(zip(s["W"], s["b"])):
                yield f"net{i}.W{l}", w
                yield f"net{i}.b{l}", b
            if s["lat"] is not None:
                yield f"net{i}.latent", s["lat"]
                yield f"net{i}.wz", s["wz"]

    def args(self, outs, null_intermediates):
        from go1_gym_learn.ppo_cse import fused as F
        a = F.TailArgs()
        a.num_nets = len(self.specs)
        for N, s, o in zip(a.net, self.specs, outs):
            dims, L = s["dims"], len(s["dims"]) - 1
            assert s["in_off"] % 8 == 0 and s["x"].ld % 8 == 0 and s["x"].ld >= s["in_off"] + dims[0]      # an accepted, in-bounds launch
            N.in_, N.rows, N.ld_in, N.num_layers = s["x"].ptr() + 2 * s["in_off"], s["rows"], s["x"].ld, L
            N.elu_in, N.npv, N.lat_ld, N.wz_ld = s["elu_in"], s["npv"], s["lat_ld"], s["wz_ld"]
            if s["lat"] is not None and s["elu_in"]:
                assert s["lat"].ld == s["lat_ld"] >= s["npv"] and s["wz"].ld == s["wz_ld"] >= s["npv"] and s["wz"].rows == dims[0]
                N.latent, N.wz = s["lat"].ptr(), s["wz"].ptr()
            for l in range(L):
                Lr = N.layer[l]
                assert s["W"][l].n == dims[l + 1] * dims[l] and s["b"][l].n == dims[l + 1] and o[l].rows == s["rows"]
                Lr.W, Lr.bias, Lr.n_out, Lr.k_in, Lr.elu = s["W"][l].ptr(), s["b"][l].ptr(), dims[l + 1], dims[l], s["elu"][l]
                if null_intermediates and l < L - 1:
                    Lr.out, Lr.ld_out = None, 0
                else:
                    Lr.out, Lr.ld_out = o[l].ptr(), o[l].ld
        return a

    def run(self, lib, null_intermediates=False):
        outs = [[Mat(s["rows"], n + s["out_pad"]) for n in s["dims"][1:]] for s in self.specs]
        before = [(name, b, b.flat.clone()) for name, b in self.inputs()]
        a = self.args(outs, null_intermediates)
        rc = lib.go1ppo_tail_fwd(ctypes.byref(a), stream())
        torch.cuda.synchronize()
        assert rc == 0
        for name, b, copy in before:
            assert same_bits(b.flat, copy), f"{name} was written"
        for i, (s, o) in enumerate(zip(self.specs, outs)):
            for l, m in enumerate(o):
                written = 0 if (null_intermediates and l < len(o) - 1) else s["dims"][l + 1]
                assert bool((m.outside(written) == 7).all()), f"net{i} layer {l}: a canary or a column >= n_out was written"
        return outs

    def twice(self, lib, null_intermediates=False):
        first, second = self.run(lib, null_intermediates), self.run(lib, null_intermediates)
        for i, (a, b) in enumerate(zip(first, second)):
            for l, (x, y) in enumerate(zip(a, b)):
                assert same_bits(x.flat, y.flat), f"net{i} layer {l}: launch 1 differs from launch 0"
        return first

    def stored(self, outs):
        """[net][layer] -> bf16 bit patterns of the n_out columns"""
        return [[host(m.m[:, :n]) for m, n in zip(o, s["dims"][1:])] for s, o in zip(self.specs, outs)]


# ------------------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("c", T.EXACT_CASES, ids=lambda c: c.name)
def test_exact_case_is_bit_for_bit(lib, c):
    nets = T.exact_inputs(c)
    run = Launch([spec(d) for d in nets])
    got = run.stored(run.twice(lib))
    wrong = total = 0
    for i, (d, st) in enumerate(zip(nets, got)):
        for l, (want, g) in enumerate(zip(T.exact_model(d), st)):
            bad = int((want != g).sum())
            print(f"\ntail_fwd_fp64 [tail exact] {c.name} net{i} layer {l} ({d['net'].dims[l]} -> {d['net'].dims[l + 1]}, {d['net'].rows} rows): "
                  f"{bad} of {g.size} differ", end="")
            wrong, total = wrong + bad, total + g.size
    note("tail exact", c.name, mismatch_share=wrong / total)
    assert wrong == 0


MULTI_LAYER = [c for c in T.EXACT_CASES if any(len(n.dims) > 2 for n in c.nets)]


@pytest.mark.parametrize("c", MULTI_LAYER + T.ROUNDED_CASES[:1], ids=lambda c: c.name)
def test_null_intermediates_leave_the_same_head(lib, c):
    """out == NULL on every layer but the last (ld_out = 0 there: not looked at): the head is bit for bit the one of the launch that
    stores everything, and nothing else is written"""
    nets = T.exact_inputs(c) if isinstance(c, T.ExactCase) else T.rounded_inputs(c)
    run = Launch([spec(d) for d in nets])
    full, null = run.twice(lib), run.twice(lib, null_intermediates=True)
    differ = sum(int(not same_bits(f[-1].flat, n[-1].flat)) for f, n in zip(full, null))
    note("tail null intermediates", c.name, heads_that_differ=float(differ))
    assert differ == 0


# ------------------------------------------------------------------------------------------------------------------ rounded cases
@pytest.mark.parametrize("c", T.ROUNDED_CASES, ids=lambda c: c.name)
def test_rounded_case_lies_inside_the_bounds(lib, c):
    nets = T.rounded_inputs(c)
    run = Launch([spec(d) for d in nets])
    got = run.stored(run.twice(lib))
    outside, share, worst = T.shares(nets, got)
    ref = T.reference_share(c)
    n = T.elements(nets)
    print(f"\ntail_fwd_fp64 [tail rounded] {c.name}: outside={outside} ratio={worst:.5f}  mismatch share: kernel {share:.6f} ({round(share * n)} of {n}), "
          f"fp32 left-to-right reference {ref:.6f} ({round(ref * n)}), cap {2 * ref:.6f}", end="")
    assert outside == 0
    note("tail rounded", c.name, ratio=worst, share_over_cap=share / (2 * ref))
    assert share <= 2 * ref


# ------------------------------------------------------------------------------------------------------------------ ELU on load
def tight(bits, npv):
    """the first npv columns as a matrix of their own (even leading dimension for npv == 2, 16-byte aligned)"""
    return mat(np.ascontiguousarray(bits[:, :npv]))


@pytest.mark.parametrize("c", T.LOAD_CASES, ids=lambda c: c.name)
def test_elu_on_load_against_the_model_and_against_elu_fwd(lib, c):
    """tail_fwd(elu_in = 1) on pre-activations: the identity layer's stored output is the activated input (the interval of the model);
    every stored output equals, bit for bit, go1ppo_elu_fwd on a copy followed by tail_fwd(elu_in = 0); the pre-activations stay"""
    nets = T.load_inputs(c)
    on_load = Launch([spec(d, elu_in=1) for d in nets])
    outs = on_load.twice(lib)                                       # (checks that x, the latent and wz are as they were)
    got = on_load.stored(outs)
    worst, mism, total = 0.0, 0, 0
    for d, st in zip(nets, got):
        v, e = T.load_model(d)
        assert T.two_valued(v, e) <= 0.01
        outside, mismatch = T.compare(st[0], v, e)
        assert not outside.any(), f"{int(outside.sum())} of {outside.size} outside their interval"
        worst, mism, total = max(worst, T.ratio_to_bound(st[0], v, e)), mism + int(mismatch.sum()), total + mismatch.size
    # the two-launch route on copies
    specs = [spec(d, elu_in=0) for d in nets]
    for s, d in zip(specs, nets):
        n = d["net"]
        x0 = s["x"].clone()
        if n.npv:
            lat, wz = (tight(d["lat"], n.npv), tight(d["wz"], n.npv)) if T.load_path(n) == "general" and n.npv == 2 else (s["lat"], s["wz"])
            assert n.npv != 2 or (lat.ld % 2 == 0 and wz.ld % 2 == 0 and lat.ptr() % 4 == 0 and wz.ptr() % 4 == 0)
            rc = lib.go1ppo_elu_fwd(s["x"].ptr(), n.rows, n.k, s["x"].ld, lat.ptr(), lat.ld, n.npv, wz.ptr(), wz.ld, n.k, stream())
        else:
            rc = lib.go1ppo_elu_fwd(s["x"].ptr(), n.rows, n.k, s["x"].ld, None, 0, 0, None, 0, 0, stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert same_bits(s["x"].outside(n.k), x0.outside(n.k)), "go1ppo_elu_fwd wrote outside its columns"
    two = Launch(specs)
    outs2 = two.twice(lib)
    for i, (a, b, s) in enumerate(zip(outs, outs2, specs)):
        for l, (x, y) in enumerate(zip(a, b)):
            assert same_bits(x.flat, y.flat), f"net{i} layer {l}: elu_in differs from go1ppo_elu_fwd + tail_fwd"
        assert same_bits(s["x"].m[:, :s["dims"][0]], a[0].m[:, :s["dims"][0]]), f"net{i}: the activated input differs from go1ppo_elu_fwd's"
    note("tail elu_in", c.name + " (" + "+".join(T.load_path(d["net"]) for d in nets) + ")", ratio=worst, mismatch_share=mism / total)


# ------------------------------------------------------------------------------------------------------------------ go1ppo_elu_fwd
@pytest.mark.parametrize("c", T.ELU_CASES, ids=lambda c: c.name)
def test_elu_fwd_kernel_matches_the_fp64_model(lib, c):
    d = T.elu_inputs(c)
    y0 = mat(d["y"])
    lat, wz = (mat(d["lat"]), mat(d["wz"])) if c.npv else (None, None)
    results = []
    for _ in (0, 1):
        y = y0.clone()
        copies = [(b, b.flat.clone()) for b in (lat, wz) if b is not None]
        if c.npv:
            assert lat.ld == c.lat_ld >= c.npv and wz.ld == c.wz_ld >= c.npv and wz.rows == c.cols >= c.lat_cols
            rc = lib.go1ppo_elu_fwd(y.ptr(), c.rows, c.cols, c.ld, lat.ptr(), c.lat_ld, c.npv, wz.ptr(), c.wz_ld, c.lat_cols, stream())
        else:
            rc = lib.go1ppo_elu_fwd(y.ptr(), c.rows, c.cols, c.ld, None, 0, 0, None, 0, 0, stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert all(same_bits(b.flat, copy) for b, copy in copies), "the latent or wz was written"
        assert same_bits(y.outside(c.cols), y0.outside(c.cols)), "a column >= cols or a canary was written"
        results.append(y)
    assert same_bits(results[0].flat, results[1].flat)
    got = host(results[0].m[:, :c.cols])
    v, e = T.elu_model(d)
    assert T.two_valued(v, e) <= 0.01
    outside, mismatch = T.compare(got, v, e)
    assert not outside.any(), f"{int(outside.sum())} of {outside.size} outside their interval"
    note("elu_fwd", c.name, ratio=T.ratio_to_bound(got, v, e), mismatch_share=float(mismatch.mean()))


# ------------------------------------------------------------------------------------------------------------------ through the engine
def test_inference_engine_equals_the_direct_c_calls(lib):
    """FusedNet(with_grad=False) at 37 rows (no multiple of 32, the fused-tails path with ELU on load) against go1ppo_tail_fwd called
    directly on the engine's own buffers with arguments built here, and against the route without ELU on load (go1ppo_elu_fwd on a
    copy of the first layer's output, then go1ppo_tail_fwd with elu_in = 0)"""
    from go1_gym_learn.ppo_cse import fused as F
    from go1_gym_learn.ppo_cse.actor_critic import ActorCritic
    from go1_gym_learn.ppo_cse.flat_policy import FlatPolicy, HEAD_COLS
    torch.manual_seed(11)
    M = 37
    ac = ActorCritic(70, 2, 2100, 12)
    pol = FlatPolicy(ac)
    flat = torch.zeros(pol.numel)
    pol.pack(ac, flat)
    body = flat.to("cuda", torch.bfloat16)
    net = F.FusedNet(pol, body, None, M, lib, with_grad=False, two_streams=False)
    assert net._tails is not None and net._elu_on_load and M % 32 and M <= 2048
    x = (0.5 * torch.randn(M, pol.Kp)).to("cuda", torch.bfloat16)
    x[:, pol.K] = 1.0
    mean, value, latent = (t.clone() for t in net.forward(x))
    torch.cuda.synchronize()
    assert float(mean.float().abs().max()) > 0 and float(value.float().abs().max()) > 0 and float(latent.float().abs().max()) > 0
    nd, na = net.nd, net.na
    y1 = net.Y1.clone()
    blocks = dict(adaptation=(0, nd), actor=(nd, na), critic=(nd + na, net.nc))
    heads = {n: net.Z[n][net.depth[n] - 1] for n in net.depth}

    def args(names, y, elu_in, latent_for=None):
        a = F.TailArgs()
        a.num_nets = len(names)
        for N, name in zip(a.net, names):
            c0, k = blocks[name]
            d = net.depth[name]
            N.in_, N.rows, N.ld_in, N.num_layers, N.elu_in = y.data_ptr() + 2 * c0, M, y.stride(0), d - 1, elu_in
            assert y.stride(0) >= c0 + k and net.P[f"{name}.1.W"].shape[1] == k
            if name == latent_for:
                lat, wz = heads["adaptation"], net.P["Wz"]
                assert tuple(wz.shape) == (k, HEAD_COLS) and tuple(lat.shape) == (M, HEAD_COLS) and pol.npv <= HEAD_COLS
                N.latent, N.wz, N.lat_ld, N.wz_ld, N.npv = lat.data_ptr(), wz.data_ptr(), lat.stride(0), wz.stride(0), pol.npv
            for li in range(1, d):
                L, W, z = N.layer[li - 1], net.P[f"{name}.{li}.W"], net.Z[name][li]
                assert tuple(z.shape) == (M, W.shape[0])
                L.W, L.bias, L.out = W.data_ptr(), net.P[f"{name}.{li}.b"].data_ptr(), z.data_ptr() if li == d - 1 else None
                L.n_out, L.k_in, L.ld_out, L.elu = W.shape[0], W.shape[1], z.stride(0), int(li < d - 1)
        return a

    def clear():
        for zs in net.Z.values():
            for z in zs.values():
                z.fill_(7.0)

    differ = {}
    # (a) the same launches, arguments built here
    clear()
    for a in (args(["adaptation"], net.Y1, 1), args(["actor", "critic"], net.Y1, 1, latent_for="actor")):
        assert lib.go1ppo_tail_fwd(ctypes.byref(a), stream()) == 0
    torch.cuda.synchronize()
    assert same_bits(net.Y1, y1), "the pre-activations were written"
    for name, want in (("actor", mean), ("critic", value), ("adaptation", latent)):
        differ[f"direct.{name}"] = float(not same_bits(heads[name], want))
    # (b) without ELU on load, on a copy of the first layer's output
    clear()
    y = y1.clone()
    assert lib.go1ppo_elu_fwd(y.data_ptr(), M, nd, y.stride(0), None, 0, 0, None, 0, 0, stream()) == 0
    a = args(["adaptation"], y, 0)
    assert lib.go1ppo_tail_fwd(ctypes.byref(a), stream()) == 0
    lat, wz = heads["adaptation"], net.P["Wz"]
    assert lib.go1ppo_elu_fwd(y.data_ptr() + 2 * nd, M, na + net.nc, y.stride(0), lat.data_ptr(), lat.stride(0), pol.npv, wz.data_ptr(), wz.stride(0), na,
                              stream()) == 0
    a = args(["actor", "critic"], y, 0)
    assert lib.go1ppo_tail_fwd(ctypes.byref(a), stream()) == 0
    torch.cuda.synchronize()
    for name, want in (("actor", mean), ("critic", value), ("adaptation", latent)):
        differ[f"two_launch.{name}"] = float(not same_bits(heads[name], want))
    note("tail engine", f"FusedNet, {M} rows", **differ)
    assert not any(differ.values()), differ
