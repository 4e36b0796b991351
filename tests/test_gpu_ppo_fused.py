"""Fused PPO-update kernels (csrc/go1ppo.hip through include/go1ppo.h) vs plain PyTorch fp32 references of the same
ops, then the hand-scheduled mini-batch (fused.py) vs the autograd path of ppo.py on identical data.

Tolerances: activations are bf16 (8 mantissa bits, eps = 3.9e-3); element-wise kernels compute in fp32 and round
once -> 1 bf16 ulp; reductions accumulate bf16-rounded terms in fp32 -> 2e-3 relative to the column's |sum| scale;
whole-network gradients are compared per parameter block by relative L2 error (two bf16 pipelines with different
rounding points): <= 3e-2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from go1_gym_learn.ppo_cse import fused
    return fused.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bf(t):
    return t.to(torch.bfloat16)


def test_elu_forward_with_latent_columns(lib):
    g = torch.Generator(device="cuda").manual_seed(0)
    M, ld, c_off, cols, lat_cols, npv = 1000, 1280, 256, 1024, 512, 2
    y = bf(torch.randn(M, ld, device="cuda", generator=g) * 2)
    lat = bf(torch.randn(M, 64, device="cuda", generator=g))
    wz = bf(torch.randn(lat_cols, 64, device="cuda", generator=g))
    ref = y.float().clone()
    blk = ref[:, c_off:c_off + cols]
    blk[:, :lat_cols] += lat[:, :npv].float() @ wz[:, :npv].float().t()
    ref[:, c_off:c_off + cols] = torch.nn.functional.elu(blk)
    view = y[:, c_off:]
    assert lib.go1ppo_elu_fwd(view.data_ptr(), M, cols, ld, lat.data_ptr(), 64, npv, wz.data_ptr(), 64, lat_cols, stream()) == 0
    torch.cuda.synchronize()
    torch.testing.assert_close(y.float(), bf(ref).float(), rtol=8e-3, atol=1e-6)        # <= 1 bf16 ulp
    assert torch.equal(y[:, :c_off], bf(ref)[:, :c_off])                                   # outside the block: untouched
    # plain ELU on a narrow matrix
    z = bf(torch.randn(333, 64, device="cuda", generator=g))
    ref = bf(torch.nn.functional.elu(z.float()))
    assert lib.go1ppo_elu_fwd(z.data_ptr(), 333, 64, 64, None, 0, 0, None, 0, 0, stream()) == 0
    torch.testing.assert_close(z.float(), ref.float(), rtol=8e-3, atol=1e-6)


@pytest.mark.parametrize("cols,ld", [(64, 64), (128, 128), (256, 256), (1024, 1280)])
def test_elu_backward_and_bias_gradient(lib, cols, ld):
    g = torch.Generator(device="cuda").manual_seed(1)
    M = 2000
    h = bf(torch.nn.functional.elu(torch.randn(M, ld, device="cuda", generator=g)))
    d = bf(torch.randn(M, ld, device="cuda", generator=g))
    hf, df = h.float()[:, :cols], d.float()[:, :cols]
    ref = bf(df * torch.where(hf > 0, torch.ones_like(hf), hf + 1.0))
    bias = torch.zeros(cols, device="cuda")
    d0 = d.clone()
    assert lib.go1ppo_elu_bwd(d.data_ptr(), ld, h.data_ptr(), ld, M, cols, bias.data_ptr(), d.data_ptr(), ld, stream()) == 0
    torch.cuda.synchronize()
    torch.testing.assert_close(d[:, :cols].float(), ref.float(), rtol=8e-3, atol=1e-6)
    assert torch.equal(d[:, cols:], d0[:, cols:])
    torch.testing.assert_close(bias, d[:, :cols].float().sum(0), rtol=1e-4, atol=1e-3)
    # identity mode = column sums only
    bias.zero_()
    d1 = d.clone()
    assert lib.go1ppo_elu_bwd(d.data_ptr(), ld, None, 0, M, cols, bias.data_ptr(), d.data_ptr(), ld, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(d, d1)
    torch.testing.assert_close(bias, d[:, :cols].float().sum(0), rtol=1e-4, atol=1e-3)
    # out of place into a column block of a wider matrix
    wide = torch.zeros(M, cols + 64, device="cuda", dtype=torch.bfloat16)
    assert lib.go1ppo_elu_bwd(d0.data_ptr(), ld, h.data_ptr(), ld, M, cols, None, wide[:, 64:].data_ptr(), cols + 64, stream()) == 0
    torch.cuda.synchronize()
    torch.testing.assert_close(wide[:, 64:].float(), ref.float(), rtol=8e-3, atol=1e-6)
    assert not wide[:, :64].any()


@pytest.mark.parametrize("M,n,k,ld_dz,ld_h", [(24576, 256, 512, 256, 1280), (24576, 64, 128, 64, 128), (5000, 512, 64, 1280, 64),
                                               (31, 64, 64, 64, 64), (24576, 128, 256, 128, 256)])
def test_wgrad_matches_fp32_matmul(lib, M, n, k, ld_dz, ld_h):
    g = torch.Generator(device="cuda").manual_seed(2)
    dz = bf(torch.randn(M, ld_dz, device="cuda", generator=g))
    h = bf(torch.randn(M, ld_h, device="cuda", generator=g))
    out = torch.full((n, k), 1.0, device="cuda")                   # accumulates on top of what is there
    bias = torch.full((n,), -2.0, device="cuda")
    assert lib.go1ppo_wgrad(dz.data_ptr(), ld_dz, h.data_ptr(), ld_h, M, n, k, out.data_ptr(), k, bias.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    ref = dz[:, :n].float().t() @ h[:, :k].float() + 1.0
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=2e-3 * M ** 0.5)      # exact bf16 products, fp32 sums
    torch.testing.assert_close(bias, dz[:, :n].float().sum(0) - 2.0, rtol=1e-4, atol=2e-3 * M ** 0.5)
    out2 = torch.zeros(n, k, device="cuda")
    assert lib.go1ppo_wgrad(dz.data_ptr(), ld_dz, h.data_ptr(), ld_h, M, n, k, out2.data_ptr(), k, None, stream()) == 0
    torch.cuda.synchronize()
    torch.testing.assert_close(out2, ref - 1.0, rtol=1e-4, atol=2e-3 * M ** 0.5)
    assert lib.go1ppo_wgrad(dz.data_ptr(), ld_dz, h.data_ptr(), ld_h, M, 48, k, out.data_ptr(), k, None, stream()) == -1


@pytest.mark.parametrize("M", [24576, 1000])
def test_mlp2_forward_and_backward_match_fp32_torch(lib, M):
    """the LDS-resident 256 -> 128 -> 64 kernels, two nets per launch with different strides, vs fp32 torch on the same
    bf16 weights / inputs.  Intermediate activations are rounded to bf16 in both (the reference below rounds where the
    kernel stores), so the comparison is 1-2 bf16 ulp of each tensor's scale."""
    import ctypes
    from go1_gym_learn.ppo_cse import fused
    g = torch.Generator(device="cuda").manual_seed(M)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    F = torch.nn.functional
    nets, fw, bw, keep = [], (fused.Mlp2Fwd * 2)(), (fused.Mlp2Bwd * 2)(), []
    for i, (ld_x, elu_input) in enumerate(((1280, 1), (256, 0))):
        xbuf = bf(rn(M, ld_x) * 1.5)
        x = xbuf[:, ld_x - 256:]                                  # a column block of a wider matrix
        W2, b2, W3, b3 = bf(rn(128, 256) / 16), bf(rn(128) * 0.1), bf(rn(64, 128) / 11), bf(rn(64) * 0.1)
        z2, out = torch.zeros(M, 128, device="cuda", dtype=torch.bfloat16), torch.full((M, 64 + 8), 3.0, device="cuda", dtype=torch.bfloat16)
        d_out = bf(rn(M, 64))
        d_z2, d_xbuf = torch.zeros(M, 128, device="cuda", dtype=torch.bfloat16), torch.full((M, 320), 5.0, device="cuda", dtype=torch.bfloat16)
        x0 = x.float().clone()
        P, Q = fw[i], bw[i]
        P.x, P.W2, P.b2, P.W3, P.b3, P.z2, P.out = x.data_ptr(), W2.data_ptr(), b2.data_ptr(), W3.data_ptr(), b3.data_ptr(), z2.data_ptr(), out.data_ptr()
        P.rows, P.ld_x, P.ld_z2, P.ld_out, P.elu_input = M, ld_x, 128, 72, elu_input
        Q.d_out, Q.z2, Q.h, Q.W2, Q.W3, Q.d_z2, Q.d_x = d_out.data_ptr(), z2.data_ptr(), x.data_ptr(), W2.data_ptr(), W3.data_ptr(), d_z2.data_ptr(), d_xbuf.data_ptr()
        Q.rows, Q.ld_dout, Q.ld_z2, Q.ld_h, Q.ld_dz2, Q.ld_dx = M, 64, 128, ld_x, 128, 320
        keep.append((xbuf, x, x0, W2, b2, W3, b3, z2, out, d_out, d_z2, d_xbuf, elu_input))
    assert lib.go1ppo_mlp2_fwd(fw, 2, stream()) == 0
    assert lib.go1ppo_mlp2_bwd(bw, 2, stream()) == 0
    torch.cuda.synchronize()
    ulp = 2.0 ** -8
    close = lambda a, b, scale: torch.testing.assert_close(a.float(), b, rtol=2 * ulp, atol=2 * ulp * scale)
    for xbuf, x, x0, W2, b2, W3, b3, z2, out, d_out, d_z2, d_xbuf, elu_input in keep:
        h0 = bf(F.elu(x0)).float() if elu_input else x0
        close(x, h0, 1.0)                                         # activated in place (or untouched)
        z2_ref = F.elu(h0 @ W2.float().t() + b2.float())
        close(z2, z2_ref, 1.0)
        out_ref = z2.float() @ W3.float().t() + b3.float()        # from the kernel's own (bf16-rounded) hidden layer
        close(out[:, :64], out_ref, 1.0)
        assert torch.all(out[:, 64:] == 3.0)
        dz2_ref = (d_out.float() @ W3.float()) * torch.where(z2.float() > 0, 1.0, z2.float() + 1.0)
        close(d_z2, dz2_ref, float(dz2_ref.abs().max()) / 4)
        dx_ref = (d_z2.float() @ W2.float()) * torch.where(x.float() > 0, 1.0, x.float() + 1.0)
        close(d_xbuf[:, :256], dx_ref, float(dx_ref.abs().max()) / 4)
        assert torch.all(d_xbuf[:, 256:] == 5.0)


def test_wgrad_tn_batched_matches_fp32_matmul(lib):
    """the 128-tile weight-gradient kernel (LDS-DMA + transpose reads), several problems of different shapes in one
    launch: first-layer sized (k = 2112: the last column tile is half empty), tails, a 64-row head, strided operands."""
    import ctypes
    from go1_gym_learn.ppo_cse import fused
    g = torch.Generator(device="cuda").manual_seed(5)
    M = 24576
    shapes = [(256, 2112, 1280, 2112, True), (256, 512, 256, 1280, True), (64, 128, 64, 128, False), (512, 64, 1280, 64, True),
              (72, 200, 80, 256, True)]
    tab = (fused.WgradProblem * len(shapes))()
    keep, refs = [], []
    for P, (n, k, ld_dz, ld_h, with_bias) in zip(tab, shapes):
        rows = M if n * k > 100000 else 4096
        dz = bf(torch.randn(rows, ld_dz, device="cuda", generator=g))
        h = bf(torch.randn(rows, ld_h, device="cuda", generator=g))
        out = torch.full((n, k), 1.0, device="cuda")
        bias = torch.full((n,), -2.0, device="cuda") if with_bias else None
        P.dz, P.h, P.dW, P.bias_grad = dz.data_ptr(), h.data_ptr(), out.data_ptr(), bias.data_ptr() if with_bias else None
        P.rows, P.ld_dz, P.ld_h, P.n, P.k, P.ldw = rows, ld_dz, ld_h, n, k, k
        keep.append((dz, h, out, bias))
        refs.append((dz[:, :n].float().t() @ h[:, :k].float() + 1.0, dz[:, :n].float().sum(0) - 2.0, rows))
    total = lib.go1ppo_wgrad_tn_plan(tab, len(shapes))
    assert total > 0
    dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
    assert lib.go1ppo_wgrad_tn_batched(dev.data_ptr(), len(shapes), total, stream()) == 0
    torch.cuda.synchronize()
    for (dz, h, out, bias), (ref, bref, rows) in zip(keep, refs):
        torch.testing.assert_close(out, ref, rtol=1e-4, atol=2e-3 * rows ** 0.5)
        if bias is not None:
            torch.testing.assert_close(bias, bref, rtol=1e-4, atol=2e-3 * rows ** 0.5)
    tab[0].rows = 1000                                             # not a multiple of 64
    assert lib.go1ppo_wgrad_tn_plan(tab, 1) == -1


@pytest.mark.parametrize("M,N,K", [(24576, 1280, 2112), (24576, 256, 2112), (4096, 128, 256), (1000, 64, 128), (130, 12, 64),
                                   (257, 388, 192)])
@pytest.mark.parametrize("epilogue", ["bias", "bias_bf16", "elu", "elu_range", "elu_skip", "elu_bwd"])
def test_gemm_nt_matches_fp32_matmul(lib, M, N, K, epilogue):
    """go1ppo_gemm_nt vs fp32 matmul of the same bf16 operands; the fp32 result is rounded to bf16 once, the kernel
    accumulates in fp32 in a different order -> 1 bf16 ulp of the pre-activation scale, plus 1 ulp of the result."""
    from go1_gym_learn.ppo_cse import fused
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    big_a = bf(torch.randn(M, K + 64, device="cuda", generator=g))
    a = big_a[:, :K]                                             # strided operand (lda > K)
    b = bf(torch.randn(N, K, device="cuda", generator=g) / K ** 0.5)
    bias = torch.randn(N, device="cuda", generator=g)
    out_full = torch.full((M, N + 16), 7.0, device="cuda", dtype=torch.bfloat16)
    c = out_full[:, :N]
    pre = a.float() @ b.float().t() + bias
    if epilogue == "bias":
        fused.gemm_nt(lib, a, b, c, bias)
        ref = pre
    elif epilogue == "bias_bf16":                                 # the parameters' bf16 compute copy as the bias (the update's 512 -> 256 layers)
        bias16 = bf(bias)
        pre = a.float() @ b.float().t() + bias16.float()
        fused.gemm_nt(lib, a, b, c, bias16)
        ref = pre
    elif epilogue == "elu_skip":
        s0, s1 = (N // 5 // 4) * 4, (3 * N // 5 // 4) * 4
        g_ = fused.gemm_args(a, b, c, bias, elu=True, elu_skip=(s0, s1))
        assert lib.go1ppo_gemm_nt(__import__("ctypes").byref(g_), stream()) == 0
        ref = torch.nn.functional.elu(pre)
        ref[:, s0:s1] = pre[:, s0:s1]
    elif epilogue == "elu":
        fused.gemm_nt(lib, a, b, c, bias, elu=True)
        ref = torch.nn.functional.elu(pre)
    elif epilogue == "elu_range":
        c0, c1 = (N // 8) * 4, N
        fused.gemm_nt(lib, a, b, c, bias, elu=(c0, c1))
        ref = pre.clone()
        ref[:, c0:c1] = torch.nn.functional.elu(pre[:, c0:c1])
    else:
        h = bf(torch.nn.functional.elu(torch.randn(M, N, device="cuda", generator=g)))
        pre = a.float() @ b.float().t()
        fused.gemm_nt(lib, a, b, c, None, elu_bwd_of=h)
        ref = pre * torch.where(h.float() > 0, torch.ones_like(pre), h.float() + 1)
    torch.cuda.synchronize()
    assert torch.all(out_full[:, N:] == 7.0), "wrote outside the N columns"
    err = (c.float() - ref).abs()
    tol = 2 ** -8 * (ref.abs() + pre.abs().clamp(min=1.0)) + 1e-6
    assert torch.all(err <= tol), f"max err {err.max().item()} at scale {ref.abs().max().item()}"


@pytest.mark.parametrize("epilogue", ["bias_bf16", "elu_bwd"])
def test_gemm_nt_pair_is_two_gemm_nt_launches(lib, epilogue):
    """go1ppo_gemm_nt_pair (blockIdx.y picks the problem): bit-identical to the two single launches, on the update's shapes — the
    actor's and critic's 512 -> 256 forward (column blocks of the shared first-layer buffer) and their 256 -> 512 input gradients."""
    from go1_gym_learn.ppo_cse import fused
    g = torch.Generator(device="cuda").manual_seed(8)
    M = 24576
    if epilogue == "bias_bf16":
        y1 = bf(torch.randn(M, 1280, device="cuda", generator=g))
        probs = [dict(a=y1[:, 256 + 512 * i:768 + 512 * i], b=bf(torch.randn(256, 512, device="cuda", generator=g) / 22),
                      bias=bf(torch.randn(256, device="cuda", generator=g))) for i in range(2)]
        shape = (M, 256)
    else:
        h = bf(torch.nn.functional.elu(torch.randn(M, 1280, device="cuda", generator=g)))
        probs = [dict(a=bf(torch.randn(M, 256, device="cuda", generator=g)), b=bf(torch.randn(512, 256, device="cuda", generator=g) / 16),
                      elu_bwd_of=h[:, 256 + 512 * i:768 + 512 * i]) for i in range(2)]
        shape = (M, 512)
    single = [torch.zeros(shape, device="cuda", dtype=torch.bfloat16) for _ in range(2)]
    paired = [torch.zeros(shape, device="cuda", dtype=torch.bfloat16) for _ in range(2)]
    for q, c in zip(probs, single):
        fused.gemm_nt(lib, q["a"], q["b"], c, q.get("bias"), elu_bwd_of=q.get("elu_bwd_of"))
    fused.gemm_nt_pair(lib, dict(c=paired[0], **probs[0]), dict(c=paired[1], **probs[1]))
    torch.cuda.synchronize()
    for s_, p_ in zip(single, paired):
        assert torch.equal(s_, p_) and float(s_.float().abs().max()) > 0.1
    # different tile grids are refused
    import ctypes
    ga = fused.gemm_args(c=paired[0], **probs[0])
    gb = fused.gemm_args(a=probs[1]["a"][:4096], b=probs[1]["b"], c=paired[1][:4096], bias=probs[1].get("bias"),
                         elu_bwd_of=None if probs[1].get("elu_bwd_of") is None else probs[1]["elu_bwd_of"][:4096])
    assert lib.go1ppo_gemm_nt_pair(ctypes.byref(ga), ctypes.byref(gb), stream()) == -7


@pytest.mark.parametrize("count,rows,cols,zero", [(4, 1280, 2112, (768, 2101, 2103)), (1, 256, 2112, (256, 2101, 2103)), (3, 40, 64, (7, 13, 30)),
                                                  (2, 16, 24, (0, 0, 0))])
def test_sum_partials_matches_torch(lib, count, rows, cols, zero):
    """go1ppo_sum_partials: fp32 sum of the bf16 row-chunk partial products of the first-layer weight gradient, with exact zeros on
    the masked column block of the leading rows (what `param.grad` of the structurally absent inputs is in the reference: nothing)."""
    g = torch.Generator(device="cuda").manual_seed(count + rows)
    part = bf(torch.randn(count, rows + 3, cols, device="cuda", generator=g))      # batch stride larger than rows x cols
    out = torch.full((rows + 1, cols), 5.0, device="cuda")
    zr, c0, c1 = zero
    assert lib.go1ppo_sum_partials(part.data_ptr(), count, part.stride(0), rows, cols, out.data_ptr(), zr, c0, c1, stream()) == 0
    torch.cuda.synchronize()
    ref = part[:, :rows].float().sum(0)
    ref[:zr, c0:c1] = 0.0
    torch.testing.assert_close(out[:rows], ref, rtol=1e-6, atol=1e-6)
    assert bool((out[:zr, c0:c1] == 0).all()) and bool((out[rows] == 5.0).all())
    assert lib.go1ppo_sum_partials(part.data_ptr(), count, part.stride(0), rows, cols + 4, out.data_ptr(), 0, 0, 0, stream()) == -1


def test_adam_keeps_transposed_copies(lib):
    """Go1PpoAdamExtras: the K-contiguous bf16 copies equal body.view(rows, cols).t() after every step that visits their weights, the
    step itself is torch.optim.Adam's; a range-restricted step that does not visit them leaves them alone."""
    from go1_gym_learn.ppo_cse import fused
    g = torch.Generator(device="cuda").manual_seed(21)
    t0 = (2048, 16, 48)
    t1 = (4096, 64, 8)
    n_body, n_std = 6000, 12
    n = n_body + 16
    master = torch.randn(n, device="cuda", generator=g) * 0.1
    master[n_body + n_std:] = 0
    ref = master.clone().requires_grad_()
    master.grad = torch.zeros_like(master)
    body = torch.zeros(n_body, device="cuda", dtype=torch.bfloat16)
    std = torch.zeros(n_std, device="cuda")
    opt = fused.FusedAdam(lib, master, body, std, n_body, 1e-3, ranges=[(0, n_body + n_std)])
    d0 = torch.full((t0[2], t0[1]), 9.0, device="cuda", dtype=torch.bfloat16)
    d1 = torch.full((t1[2], t1[1]), 9.0, device="cuda", dtype=torch.bfloat16)
    opt.set_transposes([(t0[0], t0[1], t0[2], d0), (t1[0], t1[1], t1[2], d1)])
    ref_opt = torch.optim.Adam([ref], lr=1e-3)
    for it in range(4):
        grad = torch.randn(n, device="cuda", generator=g)
        grad[n_body + n_std:] = 0
        master.grad.copy_(grad)
        opt.step_(zero_grad=True)
        ref.grad = grad.clone()
        ref_opt.step()
        torch.cuda.synchronize()
        torch.testing.assert_close(master, ref.detach(), rtol=2e-5, atol=2e-7)
        assert bool((master.grad[:n_body + n_std] == 0).all())
        for (st, r, c), d in ((t0, d0), (t1, d1)):
            assert torch.equal(d, body[st:st + r * c].view(r, c).t().contiguous())
    torch.testing.assert_close(body.float(), bf(master[:n_body]).float(), rtol=0, atol=0)
    keep = d0.clone()
    sub = fused.FusedAdam(lib, master, body, std, n_body, 1e-3, ranges=[(0, 1000)])
    sub.set_transposes([(t0[0], t0[1], t0[2], d0)])
    master.grad.normal_(generator=g)
    sub.step_()
    torch.cuda.synchronize()
    assert torch.equal(d0, keep)


@pytest.mark.parametrize("tn", [True, False])
def test_batched_weight_gradient_structural_zeros(lib, tn):
    """Go1PpoWgradProblem.zero_*: the masked block of dW receives NOTHING (it keeps the value the buffer held), every other element is the
    plain product — on both batched kernels (128-tile LDS-DMA kernel / 64-tile fallback)."""
    from go1_gym_learn.ppo_cse import fused
    g = torch.Generator(device="cuda").manual_seed(5)
    M, n, k = 4096, 256, 192
    dz = bf(torch.randn(M, n, device="cuda", generator=g))
    h = bf(torch.randn(M, k, device="cuda", generator=g))
    out = torch.zeros(n, k, device="cuda")
    zn, z0, z1 = 200, 130, 133
    out[:zn, z0:z1] = 42.0
    tab = (fused.WgradProblem * 1)()
    P = tab[0]
    P.dz, P.h, P.dW, P.bias_grad = dz.data_ptr(), h.data_ptr(), out.data_ptr(), None
    P.rows, P.ld_dz, P.ld_h, P.n, P.k, P.ldw = M, n, k, n, k, k
    P.zero_n, P.zero_k0, P.zero_k1 = zn, z0, z1
    total = (lib.go1ppo_wgrad_tn_plan if tn else lib.go1ppo_wgrad_plan)(tab, 1)
    assert total > 0
    dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
    assert (lib.go1ppo_wgrad_tn_batched if tn else lib.go1ppo_wgrad_batched)(dev.data_ptr(), 1, total, stream()) == 0
    torch.cuda.synchronize()
    ref = dz.float().t() @ h.float()
    mask = torch.zeros(n, k, dtype=torch.bool, device="cuda")
    mask[:zn, z0:z1] = True
    assert bool((out[mask] == 42.0).all())
    torch.testing.assert_close(out[~mask], ref[~mask], rtol=2e-3, atol=2e-3 * float(ref.abs().max()))


def test_weight_gradient_slabs_and_their_reduction(lib):
    """Go1PpoWgradProblem.partials: every row chunk's partial tile goes into its slab with plain stores; go1ppo_grad_reduce sums the
    slabs (fp32, fixed order: two runs are bit-identical) and the bf16 row-chunk products of a library GEMM into the flat gradient,
    with the structural zeros; go1ppo_opt_prestep_pieces does the same inside the norm pass — the partials it leaves add up to the
    squared norm of the WHOLE gradient (summed pieces and plain elements alike)."""
    from go1_gym_learn.ppo_cse import fused
    g = torch.Generator(device="cuda").manual_seed(31)
    M = 8192
    flat = torch.zeros(200000, device="cuda")
    plain = torch.randn(flat.numel(), device="cuda", generator=g)
    shapes = [(256, 192, 1024, (200, 130, 133)), (64, 128, 66560, (0, 0, 0)), (24, 40, 120000, (0, 0, 0))]      # (n, k, offset in the flat gradient, mask)
    tab = (fused.WgradProblem * len(shapes))()
    keep, refs = [], []
    for P, (n, k, off, zero) in zip(tab, shapes):
        dz, h = bf(torch.randn(M, n, device="cuda", generator=g)), bf(torch.randn(M, k, device="cuda", generator=g))
        keep.append((dz, h))
        P.dz, P.h, P.dW, P.bias_grad = dz.data_ptr(), h.data_ptr(), flat[off:].data_ptr(), None
        P.rows, P.ld_dz, P.ld_h, P.n, P.k, P.ldw = M, n, k, n, k, k
        P.zero_n, P.zero_k0, P.zero_k1 = zero
        P.partials, P.partial_stride = 16, n * k                  # placeholder: the plan depends on whether a problem has slabs (256-wide tiles), not where
        ref = dz.float().t() @ h.float()
        ref[:zero[0], zero[1]:zero[2]] = 0
        refs.append(ref)
    total = lib.go1ppo_wgrad_tn_plan(tab, len(shapes))
    assert total > 0
    pieces = []
    for P, (n, k, off, zero) in zip(tab, shapes):
        S = -(-P.rows // P.chunk_rows)
        ws = torch.zeros(S, n * k, device="cuda")
        keep.append(ws)
        P.partials, P.partial_stride = ws.data_ptr(), n * k
        pieces.append((off, n * k, ws.data_ptr(), n * k, 1, S, k, (0, 0, 0)))
    assert lib.go1ppo_wgrad_tn_plan(tab, len(shapes)) == total
    # a bf16 piece: 3 row-chunk products of a (40 x 64) block, structural zeros on rows < 7, columns [13, 30)
    part = bf(torch.randn(3, 40, 64, device="cuda", generator=g))
    pieces.append((150000, 40 * 64, part.data_ptr(), 40 * 64, 2, 3, 64, (7, 13, 30)))
    ref_b = part.float().sum(0)
    ref_b[:7, 13:30] = 0
    pieces.sort()
    arr = (fused.GradPiece * len(pieces))()
    for A, (begin, count, src, stride, kind, slabs, cols, zero) in zip(arr, pieces):
        A.begin, A.count, A.src, A.stride, A.kind, A.slabs, A.cols = begin, count, src, stride, kind, slabs, cols
        A.zero_rows, A.zero_c0, A.zero_c1 = zero
    dev_tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
    dev_pieces = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    in_piece = torch.zeros(flat.numel(), dtype=torch.bool, device="cuda")
    for begin, count, *_ in pieces:
        in_piece[begin:begin + count] = True

    def run(reduce):
        flat.copy_(plain)
        assert lib.go1ppo_wgrad_tn_batched(dev_tab.data_ptr(), len(shapes), total, stream()) == 0
        reduce()
        torch.cuda.synchronize()
        return flat.clone()
    a = run(lambda: lib.go1ppo_grad_reduce(flat.data_ptr(), dev_pieces.data_ptr(), len(pieces), stream()))
    a2 = run(lambda: lib.go1ppo_grad_reduce(flat.data_ptr(), dev_pieces.data_ptr(), len(pieces), stream()))
    assert torch.equal(a, a2)                                    # fixed summation order
    assert torch.equal(a[~in_piece], plain[~in_piece])           # nothing outside the pieces is touched
    for (n, k, off, zero), ref in zip(shapes, refs):
        got = a[off:off + n * k].view(n, k)
        torch.testing.assert_close(got, ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()))
        assert bool((got[:zero[0], zero[1]:zero[2]] == 0).all())
    torch.testing.assert_close(a[150000:150000 + 40 * 64].view(40, 64), ref_b, rtol=1e-6, atol=1e-6)
    # the same sums inside the optimiser's norm pass (n_norm in front of the last plain elements: they are not counted)
    n_norm, gscale = 190001, 0.5
    partial = torch.zeros(lib.go1ppo_opt_partials(), device="cuda")
    step, lr = torch.zeros(1, device="cuda"), torch.full((1,), 1e-3, device="cuda")
    b = run(lambda: lib.go1ppo_opt_prestep_pieces(flat.data_ptr(), n_norm, dev_pieces.data_ptr(), len(pieces), gscale, partial.data_ptr(),
                                                  step.data_ptr(), lr.data_ptr(), None, 1.0, 0.01, 1e-5, 1e-2, stream()))
    assert torch.equal(a, b)
    want = float((a[:n_norm].double() * gscale).square().sum())
    assert abs(float(partial.double().sum()) - want) <= 1e-5 * want
    assert float(step) == 1.0


def test_adam_vector_path_is_the_scalar_path(lib):
    """go1ppo_opt_adam takes four elements per lane when both ranges start and end on multiples of four; the same step through the
    general one-element path (ranges cut off the four-element grid) gives the same parameters, moments, compute copies, fp32 tail
    and transposed copies (to the last bits: rtol 2e-6) — including a body end and a transposed block that are not multiples of four."""
    from go1_gym_learn.ppo_cse import fused
    g = torch.Generator(device="cuda").manual_seed(77)
    n_body, n_std, n = 9998, 12, 10016
    tr = (4002, 50, 27)
    results = []
    for ranges in ([(0, 6000), (6000, 4012)], [(0, 6001), (6001, 4011)]):          # vector path / scalar path over the same elements
        gg = torch.Generator(device="cuda").manual_seed(78)
        master = torch.randn(n, device="cuda", generator=gg) * 0.1
        master.grad = torch.zeros_like(master)
        body = torch.zeros(n_body, device="cuda", dtype=torch.bfloat16)
        std = torch.zeros(n_std, device="cuda")
        opt = fused.FusedAdam(lib, master, body, std, n_body, 1e-3, ranges=ranges)
        d = torch.full((tr[2], tr[1]), 9.0, device="cuda", dtype=torch.bfloat16)
        opt.set_transposes([(tr[0], tr[1], tr[2], d)])
        for it in range(3):
            master.grad.normal_(generator=gg)
            opt.step_(max_norm=1.0, zero_grad=True)
        torch.cuda.synchronize()
        assert torch.equal(d, body[tr[0]:tr[0] + tr[1] * tr[2]].view(tr[1], tr[2]).t().contiguous())
        assert bool((master.grad[:n_body + n_std + 2] == 0).all())
        results.append((master.clone(), opt.m.clone(), opt.v.clone(), body.clone(), std.clone(), d.clone()))
    for x, y in zip(*results):           # (not bit-identical: the compiler contracts the two instantiations' multiply-adds differently)
        torch.testing.assert_close(x.float(), y.float(), rtol=2e-6, atol=1e-9)


@pytest.mark.parametrize("M", [4096, 1000, 24576])
def test_fused_tail_forward_matches_layerwise_torch(lib, M):
    """go1ppo_tail_fwd (three layers, activations on chip) vs addmm + ELU per layer in fp32 on the same bf16 data."""
    import ctypes
    from go1_gym_learn.ppo_cse import fused
    g = torch.Generator(device="cuda").manual_seed(9)
    ld_in, off = 1280, 256
    y1 = bf(torch.randn(M, ld_in, device="cuda", generator=g))
    nets = {"actor": (off, [512, 256, 128, 64]), "critic": (off + 512, [512, 256, 128, 64])}
    a = fused.TailArgs()
    a.num_nets = 2
    keep, refs = [], {}
    for N, (name, (o, dims)) in zip(a.net, nets.items()):
        h = y1[:, o:o + dims[0]]
        N.in_, N.rows, N.ld_in, N.num_layers = h.data_ptr(), M, ld_in, len(dims) - 1
        x = h.float()
        for li in range(1, len(dims)):
            W = bf(torch.randn(dims[li], dims[li - 1], device="cuda", generator=g) / dims[li - 1] ** 0.5)
            b = bf(torch.randn(dims[li], device="cuda", generator=g) * 0.1)
            out = torch.zeros(M, dims[li], device="cuda", dtype=torch.bfloat16)
            last = li == len(dims) - 1
            L = N.layer[li - 1]
            L.W, L.bias, L.out, L.n_out, L.k_in, L.ld_out, L.elu = W.data_ptr(), b.data_ptr(), out.data_ptr(), dims[li], dims[li - 1], dims[li], 0 if last else 1
            x = x @ W.float().t() + b.float()
            if not last:
                x = torch.nn.functional.elu(x)
            x = bf(x).float()                       # the kernel rounds every layer's output to bf16 once
            keep += [W, b, out]
            refs[(name, li)] = (out, x)
    assert lib.go1ppo_tail_fwd(ctypes.byref(a), stream()) == 0
    torch.cuda.synchronize()
    for (name, li), (out, ref) in refs.items():
        # one bf16 ulp per layer, compounding through <= 3 layers of O(1) activations
        torch.testing.assert_close(out.float(), ref, rtol=2e-2, atol=2e-2, msg=f"{name} layer {li}")
        assert float((out.float() - ref).abs().mean()) < 2e-3
    bad = fused.TailArgs()
    bad.num_nets = 1
    assert lib.go1ppo_tail_fwd(ctypes.byref(bad), stream()) == -1


def autograd_losses(mean, value, std, b, A):
    from go1_gym_learn.ppo_cse.ppo import gaussian_log_prob, gaussian_entropy
    logp = gaussian_log_prob(b["actions"], mean, std)
    entropy = gaussian_entropy(std)
    kl = torch.sum(torch.log(std / b["sigma"] + 1.e-5) + (b["sigma"] ** 2 + (b["mu"] - mean) ** 2) / (2.0 * std ** 2) - 0.5, axis=-1).mean()
    ratio = torch.exp(logp - b["logp"].squeeze())
    adv = b["adv"].squeeze()
    sur = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - A.clip_param, 1.0 + A.clip_param)).mean()
    vc = b["values"] + (value - b["values"]).clamp(-A.clip_param, A.clip_param)
    vl = torch.max((value - b["returns"]).pow(2), (vc - b["returns"]).pow(2)).mean()
    return sur + A.value_loss_coef * vl - A.entropy_coef * entropy, sur, vl, kl


def test_loss_kernel_matches_autograd(lib):
    from go1_gym_learn.ppo_cse import fused
    from go1_gym_learn.ppo_cse.ppo import PPO_Args as A
    g = torch.Generator(device="cuda").manual_seed(3)
    R, M, na = 9000, 4096, 12                       # storage rows, mini-batch rows
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    store = dict(actions=rnd(R, na), mu=rnd(R, na) * 0.3, sigma=torch.rand(R, na, device="cuda", generator=g) + 0.5,
                 logp=rnd(R, 1) * 0.5 - 14.0, adv=rnd(R, 1), returns=rnd(R, 1), values=rnd(R, 1))
    idx = torch.randperm(R, device="cuda", generator=g)[:M]
    mean_b = torch.zeros(M, 64, device="cuda", dtype=torch.bfloat16)
    mean_b[:, :na] = bf(store["mu"][idx] + 0.05 * rnd(M, na))
    value_b = torch.zeros(M, 64, device="cuda", dtype=torch.bfloat16)
    value_b[:, :1] = bf(store["values"][idx] + 0.3 * rnd(M, 1))          # some inside, some outside the value clip
    std = (torch.rand(na, device="cuda", generator=g) + 0.6)
    # make the old log-prob consistent with a policy close to the new one so that ratios straddle the clip range
    from go1_gym_learn.ppo_cse.ppo import gaussian_log_prob
    store["logp"][idx] = (gaussian_log_prob(store["actions"][idx], mean_b[:, :na].float(), std) + 0.15 * rnd(M)).unsqueeze(1)
    mean = mean_b[:, :na].float().requires_grad_()
    value = value_b[:, :1].float().requires_grad_()
    std_r = std.clone().requires_grad_()
    b = {k: v[idx] for k, v in store.items()}
    loss, sur, vl, kl = autograd_losses(mean, value, std_r, b, A)
    loss.backward()
    a = fused.LossArgs()
    dmean = torch.zeros(M, 64, device="cuda", dtype=torch.bfloat16)
    dvalue = torch.zeros(M, 64, device="cuda", dtype=torch.bfloat16)
    out = torch.zeros(3 + 2 * na + 1, device="cuda")           # sur, vl, kl, dstd[na], dmb[na], dvb
    a.mean, a.value, a.std, a.head_ld, a.num_actions, a.rows = mean_b.data_ptr(), value_b.data_ptr(), std.data_ptr(), 64, na, M
    a.idx = idx.data_ptr()
    a.actions, a.old_mu, a.old_sigma = store["actions"].data_ptr(), store["mu"].data_ptr(), store["sigma"].data_ptr()
    a.old_logp, a.advantages, a.returns, a.old_values = (store[k].data_ptr() for k in ("logp", "adv", "returns", "values"))
    a.clip_param, a.value_loss_coef, a.entropy_coef, a.use_clipped_value_loss = A.clip_param, A.value_loss_coef, A.entropy_coef, 1
    a.d_mean, a.d_value = dmean.data_ptr(), dvalue.data_ptr()
    a.surrogate_loss, a.value_loss, a.kl = out[0:].data_ptr(), out[1:].data_ptr(), out[2:].data_ptr()
    a.d_std, a.d_mean_bias, a.d_value_bias = out[3:].data_ptr(), out[3 + na:].data_ptr(), out[3 + 2 * na:].data_ptr()
    assert lib.go1ppo_loss(a, stream()) == 0
    torch.cuda.synchronize()
    np.testing.assert_allclose(out[:3].cpu().numpy(), [float(sur), float(vl), float(kl)], rtol=2e-4)
    torch.testing.assert_close(out[3:3 + na], std_r.grad, rtol=2e-3, atol=2e-5)
    # per-sample gradients: bf16-rounded copies of the autograd values
    torch.testing.assert_close(dmean[:, :na].float(), mean.grad, rtol=8e-3, atol=1e-9)
    torch.testing.assert_close(dvalue[:, :1].float(), value.grad, rtol=8e-3, atol=1e-9)
    assert not dmean[:, na:].any() and not dvalue[:, 1:].any()
    torch.testing.assert_close(out[3 + na:3 + 2 * na], dmean[:, :na].float().sum(0), rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(out[3 + 2 * na], dvalue[:, 0].float().sum(), rtol=1e-3, atol=1e-6)
    frac_clipped = float(((torch.exp(gaussian_log_prob(b["actions"], mean.detach(), std) - b["logp"].squeeze()) - 1).abs() > A.clip_param).float().mean())
    assert 0.05 < frac_clipped < 0.95                                           # both branches were exercised


@pytest.mark.parametrize("selective", [0, 1])
def test_mse_kernel_matches_autograd(lib, selective):
    g = torch.Generator(device="cuda").manual_seed(4)
    R, M, npv = 5000, 2000, 2
    target = torch.randn(R, npv, device="cuda", generator=g)
    idx = torch.randperm(R, device="cuda", generator=g)[:M]
    pred_b = torch.zeros(M, 64, device="cuda", dtype=torch.bfloat16)
    pred_b[:, :npv] = bf(torch.randn(M, npv, device="cuda", generator=g))
    num_train = M // 5 * 4
    sel = 0 if selective else slice(None)
    pred = pred_b[:, :npv].float().requires_grad_()
    t = target[idx]
    loss = torch.nn.functional.mse_loss(pred[:num_train, sel], t[:num_train, sel])
    test = torch.nn.functional.mse_loss(pred[num_train:, sel], t[num_train:, sel])
    loss.backward()
    d = torch.full((M, 64), 7.0, device="cuda", dtype=torch.bfloat16)
    d[:, npv:] = 0
    out = torch.zeros(2 + npv, device="cuda")
    assert lib.go1ppo_mse(pred_b.data_ptr(), 64, target.data_ptr(), npv, idx.data_ptr(), M, num_train, selective, d.data_ptr(),
                          out[2:].data_ptr(), out[0:].data_ptr(), out[1:].data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    np.testing.assert_allclose(out[:2].cpu().numpy(), [float(loss), float(test)], rtol=2e-4)
    torch.testing.assert_close(d[:, :npv].float(), pred.grad, rtol=8e-3, atol=1e-9)
    torch.testing.assert_close(out[2:], d[:, :npv].float().sum(0), rtol=1e-3, atol=1e-6)


def test_rollout_glue_kernels_match_torch(lib):
    """go1ppo_act / go1ppo_store_step / go1ppo_gae / go1ppo_normalize vs the torch statements of ppo.py / rollout_storage.py."""
    from go1_gym_learn.ppo_cse import fused
    from go1_gym_learn.ppo_cse.ppo import gaussian_log_prob
    from go1_gym_learn.ppo_cse.rollout_storage import RolloutStorage
    g = torch.Generator(device="cuda").manual_seed(6)
    N, T, A = 1000, 7, 12
    st = RolloutStorage(N, T, [70], [2], [2100], [A], "cuda:0", history_dtype=torch.bfloat16, history_pad_to=8, augment=True)
    ref = RolloutStorage(N, T, [70], [2], [2100], [A], "cuda:0", history_dtype=torch.bfloat16, history_pad_to=8, augment=True)
    std = torch.rand(A, device="cuda", generator=g) + 0.5
    for s_ in range(T):
        mean = torch.zeros(N, 64, device="cuda", dtype=torch.bfloat16)
        value = torch.zeros(N, 64, device="cuda", dtype=torch.bfloat16)
        mean[:, :A] = bf(torch.randn(N, A, device="cuda", generator=g))
        value[:, :1] = bf(torch.randn(N, 1, device="cuda", generator=g))
        noise = torch.randn(N, A, device="cuda", generator=g)
        fused.act(lib, mean, value, std, noise, st, s_)
        m = mean[:, :A].float()
        a = m + std * noise
        ref.actions[s_], ref.mu[s_], ref.sigma[s_], ref.values[s_] = a, m, std.expand_as(m), value[:, :1].float()
        ref.actions_log_prob[s_] = gaussian_log_prob(a, m, std).unsqueeze(1)
        rew = torch.randn(N, device="cuda", generator=g)
        dones = (torch.rand(N, device="cuda", generator=g) < 0.1).to(torch.uint8)
        tos = (torch.rand(N, device="cuda", generator=g) < 0.05)
        bins = torch.randint(0, 4000, (N,), device="cuda", generator=g, dtype=torch.int32)
        fused.store_step(lib, st, s_, rew, dones, tos.view(torch.uint8), bins, 0.99)
        ref.rewards[s_] = (rew + 0.99 * (ref.values[s_].squeeze(1) * tos)).unsqueeze(1)
        ref.dones[s_], ref.env_bins[s_] = dones.unsqueeze(1), bins.float().unsqueeze(1)
    torch.cuda.synchronize()
    for k in ("actions", "mu", "sigma", "values", "rewards", "env_bins"):
        torch.testing.assert_close(getattr(st, k), getattr(ref, k), rtol=1e-6, atol=1e-6, msg=k)
    torch.testing.assert_close(st.actions_log_prob, ref.actions_log_prob, rtol=1e-5, atol=1e-5)
    assert torch.equal(st.dones, ref.dones)
    last = torch.randn(N, 1, device="cuda", generator=g)
    adv_ptr = st.advantages.data_ptr()
    st.compute_returns(last, 0.99, 0.95, fused_lib=lib)
    ref.compute_returns(last, 0.99, 0.95)
    torch.cuda.synchronize()
    assert st.advantages.data_ptr() == adv_ptr and ref.advantages.data_ptr() != 0      # in place: graphs hold the address
    torch.testing.assert_close(st.returns, ref.returns, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(st.advantages, ref.advantages, rtol=1e-4, atol=1e-5)


def test_fused_adam_matches_torch_adam(lib):
    """clip_grad_norm_ + KL-adaptive lr + torch.optim.Adam over 5 steps == go1ppo_opt_prestep + go1ppo_opt_adam."""
    from go1_gym_learn.ppo_cse import fused
    g = torch.Generator(device="cuda").manual_seed(8)
    n_body, n_std = 100000, 12
    n = n_body + 16
    master = torch.randn(n, device="cuda", generator=g) * 0.1
    master[n_body + n_std:] = 0
    ref = master.clone().requires_grad_()
    master.grad = torch.zeros_like(master)
    body = torch.zeros(n_body, device="cuda", dtype=torch.bfloat16)
    std = torch.zeros(n_std, device="cuda")
    opt = fused.FusedAdam(lib, master, body, std, n_body, 1e-3, ranges=[(0, n_body + n_std)])
    opt_sub = fused.FusedAdam(lib, master.clone(), body.clone(), std.clone(), n_body, 1e-3, ranges=[(1000, 500), (70000, 64)])
    opt_sub.master.grad = torch.ones_like(master)
    ref_opt = torch.optim.Adam([ref], lr=1e-3)
    lr = 1e-3
    kl = torch.zeros(1, device="cuda")
    for it, k in enumerate([0.05, 0.001, 0.012, 0.03, 0.004]):
        grad = torch.randn(n, device="cuda", generator=g) * (3.0 if it % 2 else 0.001)      # clipped and unclipped steps
        grad[n_body + n_std:] = 0
        master.grad.copy_(grad)
        kl.fill_(k)
        opt.step_(gscale=0.5, max_norm=1.0, kl=kl, kl_scale=1.0, desired_kl=0.01)
        if k > 0.02:
            lr = max(1e-5, lr / 1.5)
        elif k < 0.005:
            lr = min(1e-2, lr * 1.5)
        ref.grad = grad * 0.5
        torch.nn.utils.clip_grad_norm_([ref], 1.0)
        for grp in ref_opt.param_groups:
            grp["lr"] = lr
        ref_opt.step()
        torch.cuda.synchronize()
        assert float(opt.lr) == pytest.approx(lr, rel=1e-6)
        torch.testing.assert_close(master, ref.detach(), rtol=2e-5, atol=2e-7)
    torch.testing.assert_close(body.float(), bf(master[:n_body]).float(), rtol=0, atol=0)
    torch.testing.assert_close(std, master[n_body:n_body + n_std], rtol=0, atol=0)
    # range-restricted optimiser touches only its elements
    before = opt_sub.master.clone()
    opt_sub.step_()
    torch.cuda.synchronize()
    changed = (opt_sub.master != before).nonzero().flatten()
    expect = torch.cat((torch.arange(1000, 1500), torch.arange(70000, 70064))).cuda()
    assert torch.equal(changed, expect)
    assert float(opt_sub.master.grad.min()) == 1.0          # zero_grad off: the gradient is left alone
    # zero_grad: exactly the visited gradient elements (and the extra slot) are cleared, the step itself is unchanged
    twin = fused.FusedAdam(lib, opt_sub.master.clone(), body.clone(), std.clone(), n_body, 1e-3, ranges=[(1000, 500), (70000, 64)])
    twin.m.copy_(opt_sub.m); twin.v.copy_(opt_sub.v); twin.step.copy_(opt_sub.step)
    twin.master.grad = torch.ones_like(master)
    slot = torch.ones(1, device="cuda")
    opt_sub.step_()
    twin.step_(zero_grad=True, zero_slot=slot)
    torch.cuda.synchronize()
    torch.testing.assert_close(twin.master, opt_sub.master, rtol=0, atol=0)
    cleared = (twin.master.grad == 0).nonzero().flatten()
    assert torch.equal(cleared, expect) and float(slot) == 0.0


def make_alg(fused_on, N, T, seed=0, bf16=True):
    from go1_gym_learn.ppo_cse.actor_critic import ActorCritic
    from go1_gym_learn.ppo_cse.ppo import PPO, PPO_Args
    PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels = bf16, fused_on
    torch.manual_seed(seed)
    alg = PPO(ActorCritic(70, 2, 2100, 12), device="cuda:0")
    alg.init_storage(N, T, [70], [2], [2100], [12])
    return alg


def fill_storage(alg, N, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for t in range(T):
        obs = torch.randn(N, 70, device="cuda", generator=g)
        priv = torch.randn(N, 2, device="cuda", generator=g)
        hist = torch.randn(N, 2100, device="cuda", generator=g)
        torch.manual_seed(1000 * seed + t)
        alg.act(obs, priv, hist)
        alg.process_env_step(torch.randn(N, device="cuda", generator=g), torch.zeros(N, dtype=torch.uint8, device="cuda"),
                             {"env_bins": torch.zeros(N, device="cuda"), "time_outs": torch.zeros(N, dtype=torch.bool, device="cuda")})
    alg.compute_returns(hist, priv)


def block_errors(pol, ga, gb):
    out = {}
    for name, _ in pol.blocks:
        a, b = pol._block(ga, name).double(), pol._block(gb, name).double()
        out[name] = float((a - b).norm() / (b.norm() + 1e-30)), float(b.norm())
    return out


@pytest.mark.parametrize("engine", ["fused_tails", "mlp2", "per_layer"])
def test_fused_minibatch_gradients_match_autograd(engine, monkeypatch):
    """Same weights, same storage, same mini-batch: the hand-scheduled backward must produce the autograd gradient
    (both bf16 pipelines) for the PPO stage and for the adaptation stage — for each of the three engines the MLP
    tails can run on (one fused forward kernel for small batches; the LDS-resident 256->128->64 kernels, forward and
    backward, for large ones; plain per-layer GEMM + ELU launches)."""
    from go1_gym_learn.ppo_cse.ppo import PPO_Args
    if engine != "fused_tails":
        monkeypatch.setenv("GO1_FUSED_TAILS_MAX_ROWS", "0")
    if engine == "per_layer":
        monkeypatch.setenv("GO1_MLP2", "0")
    N, T = 1024, 8
    algs = []
    for fused_on in (False, True):
        alg = make_alg(fused_on, N, T)
        fill_storage(alg, N, T, seed=5)
        algs.append(alg)
    PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels = False, True
    ref, fus = algs
    assert fus.fused and not ref.fused and fus._roll_net is not None
    # rollouts: the fused inference engine and FlatPolicy.forward agree
    torch.testing.assert_close(fus.storage.mu, ref.storage.mu, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(fus.storage.values, ref.storage.values, rtol=2e-2, atol=2e-2)
    # identical inputs for the update comparison
    for k in ("actions", "values", "mu", "sigma", "actions_log_prob", "advantages", "returns", "observation_histories", "privileged_observations"):
        getattr(fus.storage, k).copy_(getattr(ref.storage, k))
    mb = N * T // 4
    idx = torch.randperm(N * T, device="cuda")[:mb]
    from go1_gym_learn.ppo_cse.fused import FusedNet
    fus._train_net = FusedNet(fus.policy, fus.body, fus.master.grad[:fus.n_body], mb, fus._fused_lib, with_grad=True)
    assert fus._train_net._mlp2 == (engine == "mlp2") and (fus._train_net._tails is not None) == (engine == "fused_tails")
    for stage in ("_stage_ppo_backward", "_stage_adapt_backward"):
        for alg in (ref, fus):
            alg._acc.zero_()
            alg.master.grad.zero_()          # (update() / the fused optimiser steps keep the flat gradient clean between stages)
            getattr(alg, stage)(idx)
        torch.cuda.synchronize()
        np.testing.assert_allclose(fus._acc.cpu().numpy(), ref._acc.cpu().numpy(), rtol=1e-2, atol=1e-6)
        if stage == "_stage_ppo_backward":
            assert float(fus._kl) == pytest.approx(float(ref._kl), rel=2e-2, abs=1e-6)
        n = ref.n_body
        errs = block_errors(ref.policy, fus.master.grad[:n], ref.master.grad[:n])
        gmax = max(v[1] for v in errs.values())
        for name, (rel, norm) in errs.items():
            if norm > 1e-3 * gmax:
                assert rel < 3e-2, (stage, name, rel, norm)
            else:            # blocks this stage does not touch (or barely): absolute
                assert rel * norm < 1e-3 * gmax, (stage, name, rel, norm)
        torch.testing.assert_close(fus.master.grad[n:], ref.master.grad[n:], rtol=2e-2, atol=1e-5)
        assert float(fus.master.grad[:n].norm()) > 0


# the arms of the trajectory tests: (fused kernels, bf16) — the bf16 autograd update first (its rollouts are the ones every arm updates on), the bf16
# fused update, and the fp32 autograd update (the path tests/test_gpu_ppo_reference.py pins on the reference's fixtures)
ARMS = ((False, True), (True, True), (False, False))
BF16_TRAJECTORY_FACTOR = 1.5


def check_weight_trajectory(w_init, w_auto, w_fused, w_fp32, lr_auto, lr_fp32, what):
    """Adam's normalised steps amplify rounding differences of small gradient entries, so the weights are compared against the distance the
    optimiser steps moved them — and the bound is MEASURED in the same test, not a constant (the review of round 4, item 6): the bf16 autograd
    update and the fp32 autograd update of the same rollouts differ by bf16's round-off and nothing else (same graph, same schedule decisions),
    d_ref = |w_bf16 - w_fp32| / |w_bf16 - w_init|.  Two correct bf16 pipelines that round at different places (the fused kernels keep fp32
    accumulators through an MLP tail, autograd rounds every layer's output) sit about sqrt(2) d_ref apart if their round-offs are independent;
    the fused update has to stay within BF16_TRAJECTORY_FACTOR x d_ref of the autograd update.  (If the fp32 run took other learning-rate
    decisions than the bf16 runs its trajectory is no yardstick: the round-3 constant 0.1 applies.)"""
    moved = float((w_auto - w_init).norm())
    assert moved > 0
    rel = float((w_fused - w_auto).norm()) / moved
    d_ref = float((w_auto - w_fp32).norm()) / moved
    same_schedule = lr_fp32 == pytest.approx(lr_auto, rel=1e-5)
    bound = BF16_TRAJECTORY_FACTOR * d_ref if same_schedule else 0.1
    print(f"[bf16 trajectory] {what}: fused vs autograd {rel:.4f}, bf16 vs fp32 autograd (d_ref) {d_ref:.4f}, same schedule {same_schedule}, bound {bound:.4f}")
    assert rel < bound, (what, rel, d_ref, same_schedule)


@pytest.mark.parametrize("use_graphs,engine", [(False, "fused_tails"), (True, "fused_tails"), (False, "mlp2"), (True, "mlp2")])
def test_fused_update_tracks_autograd_update(use_graphs, engine, monkeypatch):
    """Two full update() calls (5 epochs x 4 mini-batches each, Adam, adaptive LR): the fused path stays close to the
    autograd path — same losses to 2 %, same learning-rate trajectory, same weight trajectory within bf16 noise."""
    from go1_gym_learn.ppo_cse.ppo import PPO_Args
    if engine == "mlp2":
        monkeypatch.setenv("GO1_FUSED_TAILS_MAX_ROWS", "0")
    N, T = 512, 8
    res, saved = [], {}
    for fused_on, bf16 in ARMS:
        PPO_Args.use_hip_graphs = use_graphs
        alg = make_alg(fused_on, N, T, bf16=bf16)
        w_init = alg.master.clone()
        for it in range(2):
            fill_storage(alg, N, T, seed=7 + it)
            if saved.get(it):  # compare the update on identical rollouts (the rollout engines differ by bf16 rounding)
                for k in ("actions", "values", "mu", "sigma", "actions_log_prob", "advantages", "returns", "observation_histories",
                          "privileged_observations"):
                    getattr(alg.storage, k).copy_(saved[it][k])
            else:
                saved[it] = {k: getattr(alg.storage, k).clone() for k in ("actions", "values", "mu", "sigma", "actions_log_prob", "advantages",
                                                                          "returns", "observation_histories", "privileged_observations")}
            torch.manual_seed(100 + it)
            losses = alg.update()
        assert bool(alg._graphs) == (use_graphs and fused_on)      # (the autograd update is captured only on request: "all")
        res.append((alg.master.clone(), losses, alg.learning_rate))
    PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels, PPO_Args.use_hip_graphs = False, True, True
    (w0, l0, lr0), (w1, l1, lr1), (w32, l32, lr32) = res
    assert lr1 == pytest.approx(lr0, rel=1e-5)          # same schedule decisions; the products round differently
    np.testing.assert_allclose(l1, l0, rtol=2e-2, atol=1e-6)
    check_weight_trajectory(w_init, w0, w1, w32, lr0, lr32, f"train.py settings, graphs={use_graphs}, {engine}")


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_fused_update_tracks_autograd_update_under_ppo_fuzz_settings(k):
    """GPU twins of tests/golden/ppo_fuzz<k>.npz: the four other PPO_Args settings the CPU fp32 path is pinned on against the
    reference (tests/test_ppo.py; fixed schedule, plain value loss, 2-3 adaptation sub-steps, selective adaptation loss, other
    clip / entropy / value coefficients, epochs, mini-batch counts, gamma / lambda) — here the bf16 fused update (own kernels: loss,
    mse, wgrad, Adam, GAE) against the bf16 autograd update on identical rollouts, two update() calls each.  Same criteria as the
    train.py-settings test above; graphs follow the default (captured when there is a single adaptation sub-step)."""
    from golden.variants import PPO_FUZZ
    from go1_gym_learn.ppo_cse.ppo import PPO_Args
    over = PPO_FUZZ[k]
    saved_args = {name: getattr(PPO_Args, name) for name in over}
    N, T = 480, 8                   # 3840 samples: mini-batches of 1280 / 1920 / 768 / 3840 rows
    res, saved = [], {}
    try:
        for name, v in over.items():
            setattr(PPO_Args, name, v)
        for fused_on, bf16 in ARMS:
            alg = make_alg(fused_on, N, T, bf16=bf16)
            w_init = alg.master.clone()
            for it in range(2):
                fill_storage(alg, N, T, seed=17 + it)      # (compute_returns inside: gamma / lam of this setting, GAE kernel vs torch)
                fields = ("actions", "values", "mu", "sigma", "actions_log_prob", "observation_histories", "privileged_observations",
                          "rewards", "dones")
                if not fused_on and not bf16:
                    for f in fields + ("advantages", "returns"):
                        getattr(alg.storage, f).copy_(saved[it][f])
                elif fused_on:
                    for f in fields:
                        getattr(alg.storage, f).copy_(saved[it][f])
                    # the GAE + normalisation kernels under this setting's gamma / lambda against the torch scan
                    alg.storage.compute_returns(saved[it]["last_values"].clone(), PPO_Args.gamma, PPO_Args.lam, fused_lib=alg._fused_lib)
                    torch.testing.assert_close(alg.storage.returns, saved[it]["returns"], rtol=1e-5, atol=1e-5)
                    torch.testing.assert_close(alg.storage.advantages, saved[it]["advantages"], rtol=1e-4, atol=1e-4)
                    for f in ("advantages", "returns"):
                        getattr(alg.storage, f).copy_(saved[it][f])
                else:
                    saved[it] = {f: getattr(alg.storage, f).clone() for f in fields + ("advantages", "returns")}
                    saved[it]["last_values"] = alg._infer(alg._last_hist)[1].clone()
                torch.manual_seed(100 + it)
                losses = alg.update()
            res.append((alg.master.clone(), losses, alg.learning_rate))
    finally:
        for name, v in saved_args.items():
            setattr(PPO_Args, name, v)
        PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels, PPO_Args.use_hip_graphs = False, True, True
    (w0, l0, lr0), (w1, l1, lr1), (w32, l32, lr32) = res
    assert lr1 == pytest.approx(lr0, rel=1e-5)
    if over.get("schedule") == "fixed":
        assert lr1 == pytest.approx(over.get("learning_rate", 1.e-3), rel=1e-6)
    np.testing.assert_allclose(l1, l0, rtol=2e-2, atol=1e-6)
    check_weight_trajectory(w_init, w0, w1, w32, lr0, lr32, f"ppo_fuzz{k}")


def test_fused_graph_replay_equals_eager_at_production_size():
    """HIP-graph replay of the fused update at the production size (4096 envs x 24 steps: 24576-row mini-batches).  Under ROCm 7.2
    torch's multi-block reductions do not replay reliably (profiles/r03_graph_reduce_repro.txt) — which is why the autograd update
    is not captured by default; the fused update has none of them, and this keeps it that way: the replayed run must differ from
    an eager run by no more than two eager runs differ from each other (atomic accumulation order; measured ratio 0.7-0.9)."""
    import os
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, "tools", "debug"))
    import graph_vs_eager as G
    from go1_gym_learn.ppo_cse.ppo import PPO_Args
    try:
        kw = dict(fused=True)
        a = G.run(False, True, 3, 4096, 24, True, **kw)
        a2 = G.run(False, True, 3, 4096, 24, True, **kw)
        b = G.run(True, True, 3, 4096, 24, True, **kw)
    finally:
        PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels, PPO_Args.use_hip_graphs = False, True, True
    assert bool(G.run.alg._graphs)
    for u in range(3):
        ee = float((a[u][0] - a2[u][0]).abs().max())
        ge = float((a[u][0] - b[u][0]).abs().max())
        # Both are maxima over 3 M Adam-amplified last-bit differences.  Round 4 (fp32 atomics in the weight-gradient kernels): 1-3e-3 each, so
        # "3 x eager-vs-eager + 1e-3" held.  Since the slabs replaced the atomics two EAGER runs are bit-reproducible (ee ~ 1e-8) while the
        # replay still takes its GEMMs through another hipBLASLt dispatch (pre-gathered operands): 1.3e-3 after three updates on one box of the
        # pool (gpurun call r5j), which the old floor of 1e-3 flagged.  An element whose gradient sits at a rounding boundary moves by one
        # learning rate per optimiser step the two runs round it differently: the floor is 4 learning rates (lr <= 1e-3 here).
        assert ge <= 3.0 * ee + 4e-3, (u, ge, ee)
        # (losses: the surrogate is a difference of O(1) terms around -0.04 — two EAGER runs differ by ~4e-5 there, the atomics' order)
        spread = np.abs(np.asarray(a[u][1][:3]) - np.asarray(a2[u][1][:3]))
        np.testing.assert_allclose(b[u][1][:3], a[u][1][:3], rtol=1e-3, atol=float(3.0 * spread.max() + 1e-4))
        assert b[u][2] == pytest.approx(a[u][2], rel=1e-5)


def test_fused_update_is_bit_reproducible_at_production_size():
    """Two runs of the product update (HIP graphs, bf16, 4096 envs x 24 steps, three updates) from the same seeds give the same bytes:
    weights, gradients, losses and learning rate.  The update's cross-workgroup sums (loss and MSE kernels, GAE statistics, the batched
    weight-gradient kernel's bias columns) are taken in a fixed order (csrc/go1ppo.hip, det_last) and the weight gradients go through
    slabs, so nothing depends on the order in which workgroups finish."""
    import os
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, "tools", "debug"))
    import graph_vs_eager as G
    from go1_gym_learn.ppo_cse.ppo import PPO_Args
    try:
        a = G.run(True, True, 3, 4096, 24, True, fused=True)
        b = G.run(True, True, 3, 4096, 24, True, fused=True)
    finally:
        PPO_Args.autocast_bf16, PPO_Args.use_fused_kernels, PPO_Args.use_hip_graphs = False, True, True
    for u in range(3):
        assert torch.equal(a[u][0], b[u][0]), (u, float((a[u][0] - b[u][0]).abs().max()))
        assert torch.equal(a[u][3], b[u][3]), (u, float((a[u][3] - b[u][3]).abs().max()))
        assert list(a[u][1]) == list(b[u][1]) and a[u][2] == b[u][2], (u, a[u][1], b[u][1])


def test_observation_ring_storage_is_bit_identical_to_the_history_block():
    """RolloutStorage(ring=True) — every observation stored once, (T + H - 1, N, 70) bf16 — against the reference layout
    (rollout_storage.py:36-38: every window stored, here (T, N, 2112) bf16): same sliding-window input stream
    (history_wrapper.py:23), then (a) the inference rows of every rollout step, (b) the stored obs / privileged obs, (c) the
    gathered mini-batch rows X of a shuffled index set — all bit for bit — and (d) two full update() calls: same losses and
    weights up to the run-to-run round-off of the update's atomic accumulations."""
    from go1_gym_learn.ppo_cse.ppo import PPO_Args
    N, T, H, no = 512, 8, 30, 70
    algs = []
    for ring in (False, True):
        alg = make_alg(True, N, T)
        if ring:
            alg.init_storage(N, T, [70], [2], [2100], [12], sliding_history=True)
        assert alg.storage.ring == ring
        algs.append(alg)
    full, ring = algs
    assert ring.storage.observation_histories is None and tuple(ring.storage.obs_ring.shape) == (T + H - 1, N, no)
    assert ring.storage.obs_ring.numel() * 4 < full.storage.observation_histories.numel()          # (T = 8: 6.5x; T = 24: 13.6x)
    g = torch.Generator(device="cuda").manual_seed(3)
    # a history that is NOT all-zero at the start of the first rollout and lives in a wider strided buffer, like the env's ring view
    wide = torch.randn(N, 2 * (H + 1) * no, device="cuda", generator=g)
    off = 3 * no
    for rollout in range(2):
        for t in range(T):
            obs = torch.randn(N, no, device="cuda", generator=g)
            priv = torch.randn(N, 2, device="cuda", generator=g)
            wide[:, off:off + (H - 1) * no] = wide[:, off + no:off + H * no].clone()       # slide, append
            wide[:, off + (H - 1) * no:off + H * no] = obs
            hist = wide[:, off:off + H * no]
            rew = torch.randn(N, device="cuda", generator=g)
            for alg in (full, ring):
                torch.manual_seed(100 * rollout + t)
                a = alg.act(obs, priv, hist)
                if alg is ring:
                    assert torch.equal(alg._X_roll, full.storage.observation_histories[t]), (rollout, t)
                    assert rollout > 0 or torch.equal(a, a_full)       # (after the first update the weights differ by its round-off)
                a_full = a.clone()
                alg.process_env_step(rew, torch.zeros(N, dtype=torch.uint8, device="cuda"),
                                     {"env_bins": torch.zeros(N, dtype=torch.int32, device="cuda"), "time_outs": torch.zeros(N, dtype=torch.bool, device="cuda")})
        for k in ("observations", "privileged_observations") + (("actions", "values", "rewards", "mu", "actions_log_prob") if rollout == 0 else ()):
            assert torch.equal(getattr(ring.storage, k), getattr(full.storage, k)), k
        idx = torch.randperm(N * T, device="cuda")[:N * T // 4]
        Xf, Xr = (torch.zeros(idx.numel(), alg.policy.Kp, device="cuda", dtype=torch.bfloat16) for alg in (full, ring))
        full._gather_rows(idx, Xf)
        ring._gather_rows(idx, Xr)
        assert torch.equal(Xf, Xr)
        out = []
        for alg in (full, ring):
            alg.compute_returns(hist, priv)
            torch.manual_seed(7 + rollout)
            out.append(alg.update())
        if rollout == 0:
            # identical inputs; the update itself sums weight gradients and losses with fp32 atomics (run-to-run round-off)
            np.testing.assert_allclose(out[1], out[0], rtol=1e-3, atol=1e-6)
            # (Adam normalises the step: an element whose tiny gradient differs in the last bits can move by ~lr per step)
            assert float((ring.master - full.master).abs().max()) < 5e-3 and float((ring.master - full.master).abs().mean()) < 2e-5


def test_adam_slice_reaching_past_the_live_parameters_leaves_the_tail_copy_alone(lib):
    """go1ppo_opt_adam over a range that extends beyond n_body + n_tail (a sharded step whose last slice covers the KL slot and the
    padding of the flat buffer): the fp32 tail copy is only written for its n_tail elements — the words behind it keep their
    sentinel — and an empty range is accepted (clears zero_slot only)."""
    n_body, n_tail, pad = 1000, 12, 52
    tot = n_body + n_tail + pad
    p = torch.randn(tot, device="cuda"); g = torch.randn(tot, device="cuda"); m = torch.zeros(tot, device="cuda"); v = torch.zeros(tot, device="cuda")
    step = torch.ones(1, device="cuda"); lr = torch.full((1,), 1e-3, device="cuda")
    body = torch.zeros(n_body, device="cuda", dtype=torch.bfloat16)
    arena = torch.full((n_tail + 64,), 777.0, device="cuda")
    slot = torch.ones(1, device="cuda")
    p0 = p.clone()
    assert lib.go1ppo_opt_adam(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 500, tot - 500, 0, 0, 1.0, None, 0.0, step.data_ptr(),
                               lr.data_ptr(), 0.9, 0.999, 1e-8, body.data_ptr(), n_body, arena.data_ptr(), n_tail, 0, slot.data_ptr(), None, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(arena[:n_tail], p[n_body:n_body + n_tail]) and bool((arena[n_tail:] == 777.0).all())
    assert torch.equal(p[:500], p0[:500]) and not torch.equal(p[500:], p0[500:]) and float(slot) == 0.0
    slot.fill_(1.0)
    assert lib.go1ppo_opt_adam(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 0, 0, 0, 1.0, None, 0.0, step.data_ptr(),
                               lr.data_ptr(), 0.9, 0.999, 1e-8, body.data_ptr(), n_body, arena.data_ptr(), n_tail, 0, slot.data_ptr(), None, stream()) == 0
    torch.cuda.synchronize()
    assert float(slot) == 0.0


def test_ring_rows_with_wide_privileged_observations(lib):
    """go1ppo_ring_step / go1ppo_ring_gather with more than 64 privileged columns (one wavefront per environment: the fp32
    privileged copy is written by a strided loop): stored rows and gathered rows carry every column."""
    N, H, no, npv = 37, 5, 6, 150
    Kp = ((H * no + 1 + npv + 63) // 64) * 64
    g = torch.Generator(device="cuda").manual_seed(5)
    obs = torch.randn(N, no, device="cuda", generator=g)
    priv = torch.randn(N, npv, device="cuda", generator=g)
    ring = bf(torch.randn(H, N, no, device="cuda", generator=g))
    ring[H - 1] = bf(obs)
    X = torch.zeros(N, Kp, device="cuda", dtype=torch.bfloat16)
    obs_store = torch.zeros(N, no, device="cuda"); priv_store = torch.zeros(N, npv, device="cuda")
    assert lib.go1ppo_ring_step(obs.data_ptr(), priv.data_ptr(), None, ring.data_ptr(), N, H, no, npv, Kp, X.data_ptr(), obs_store.data_ptr(),
                                priv_store.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(priv_store, priv) and torch.equal(obs_store, obs)
    want = torch.zeros(N, Kp, device="cuda", dtype=torch.bfloat16)
    want[:, :H * no] = ring.permute(1, 0, 2).reshape(N, H * no)
    want[:, H * no] = 1.0
    want[:, H * no + 1:H * no + 1 + npv] = bf(priv)
    assert torch.equal(X, want)
    idx = torch.arange(N, device="cuda", dtype=torch.int64).flip(0).contiguous()
    Xg = torch.zeros(N, Kp, device="cuda", dtype=torch.bfloat16)
    assert lib.go1ppo_ring_gather(ring.data_ptr(), priv_store.data_ptr(), idx.data_ptr(), N, N, H, no, npv, Kp, Xg.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(Xg, want.flip(0))
