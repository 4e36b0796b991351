"""Store paths of the PPO kernels (csrc/go1ppo.hip, go1ppo_gemm.h, go1ppo_mlp.h): some large outputs leave as 16-byte write-through
stores (put16_wt: the ELU pass, mlp2_bwd), the batched weight gradient's slab tiles as whole rows through LDS (wtn_slab_rows); the other
kernels here are candidates for the same that kept their plain stores.  A widened or re-shaped store
breaks the bytes AROUND the logical output first, so every output here lies inside a canary-filled buffer — in front, behind and in
the padding between `cols` and `ld` — and every test asserts that no byte outside the logical output changed.  Shapes are the smallest
that reach every store path: partial row tiles, partial column groups, more than one workgroup, both weight-gradient tile shapes.

Expected values come from fp32 / fp64 torch models with the tolerances of tests/test_gpu_ppo_fused.py for the same kernels:
element-wise kernels round once to bf16 (1 ulp: rtol 8e-3); GEMMs 2^-8 of the pre-activation scale; weight gradients are exact bf16
products summed in fp32 (rtol 1e-4, atol 2e-3 sqrt(rows)); Adam rtol 2e-5."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 512                      # canary elements in front of and behind every guarded buffer
F = torch.nn.functional


@pytest.fixture(scope="module")
def lib():
    from go1_gym_learn.ppo_cse import fused
    return fused.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bf(t):
    return t.to(torch.bfloat16)


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


class Guarded:
    """a (rows x ld) matrix inside a canary-filled flat buffer; `check(cols)`: every element outside [:, :cols] still holds its canary bits"""

    def __init__(self, rows, ld, dtype, fill=7.0, init=None):
        self.flat = torch.full((PAD + rows * ld + PAD,), fill, dtype=dtype, device="cuda")
        self.m = self.flat[PAD:PAD + rows * ld].view(rows, ld)
        if init is not None:
            self.m[:, :init.shape[1]] = init
        self.before = self.flat.clone()
        self.rows, self.ld = rows, ld

    def check(self, cols, row_mask=None):
        bits = torch.int16 if self.flat.element_size() == 2 else torch.int32
        outside = torch.ones(self.flat.numel(), dtype=torch.bool, device="cuda")
        inner = outside[PAD:PAD + self.rows * self.ld].view(self.rows, self.ld)
        inner[:, :cols] = False
        if row_mask is not None:                       # logical elements that must keep their value as well
            inner[:, :cols] |= row_mask
        a, b = self.flat.view(bits)[outside], self.before.view(bits)[outside]
        assert torch.equal(a, b), f"{int((a != b).sum())} elements outside the logical output changed"


def elu_prime(h):
    return torch.where(h > 0, torch.ones_like(h), h + 1.0)


# ------------------------------------------------------------------------------------------------------------------ ELU
@pytest.mark.parametrize("rows", [1, 63, 65, 130])
@pytest.mark.parametrize("cols,ld", [(8, 24), (136, 160)])
def test_elu_forward_in_place(lib, rows, cols, ld):
    g = gen(rows + cols)
    y = Guarded(rows, ld, torch.bfloat16, init=bf(torch.randn(rows, cols, device="cuda", generator=g) * 2))
    x0 = y.m[:, :cols].float().clone()
    assert lib.go1ppo_elu_fwd(y.m.data_ptr(), rows, cols, ld, None, 0, 0, None, 0, 0, stream()) == 0
    torch.cuda.synchronize()
    torch.testing.assert_close(y.m[:, :cols].float(), bf(F.elu(x0)).float(), rtol=8e-3, atol=1e-6)
    y.check(cols)
    # with the latent columns (npv = 2: the dword path) on the first 8 columns
    lat = bf(torch.randn(rows, 8, device="cuda", generator=g))
    wz = bf(torch.randn(cols, 8, device="cuda", generator=g))
    z = Guarded(rows, ld, torch.bfloat16, init=bf(x0))
    assert lib.go1ppo_elu_fwd(z.m.data_ptr(), rows, cols, ld, lat.data_ptr(), 8, 2, wz.data_ptr(), 8, 8, stream()) == 0
    torch.cuda.synchronize()
    ref = bf(x0).float()
    ref[:, :8] += lat[:, :2].float() @ wz[:8, :2].float().t()
    torch.testing.assert_close(z.m[:, :cols].float(), bf(F.elu(ref)).float(), rtol=8e-3, atol=1e-6)
    z.check(cols)


@pytest.mark.parametrize("rows", [1, 63, 65, 130])
@pytest.mark.parametrize("cols,ld", [(8, 24), (136, 160)])
@pytest.mark.parametrize("mode", ["in_place_sums", "out_of_place_tile", "out_of_place_sums"])
def test_elu_backward(lib, rows, cols, ld, mode):
    g = gen(3 * rows + cols)
    h = bf(F.elu(torch.randn(rows, ld, device="cuda", generator=g)))
    d = Guarded(rows, ld, torch.bfloat16, init=bf(torch.randn(rows, cols, device="cuda", generator=g)))
    d0 = d.m[:, :cols].float().clone()
    ref = bf(d0 * elu_prime(h[:, :cols].float())).float()
    bias = torch.zeros(cols, device="cuda")
    if mode == "in_place_sums":
        out = d
        assert lib.go1ppo_elu_bwd(d.m.data_ptr(), ld, h.data_ptr(), ld, rows, cols, bias.data_ptr(), d.m.data_ptr(), ld, stream()) == 0
    else:
        out = Guarded(rows, ld + 8, torch.bfloat16)
        bg = bias.data_ptr() if mode == "out_of_place_sums" else None
        assert lib.go1ppo_elu_bwd(d.m.data_ptr(), ld, h.data_ptr(), ld, rows, cols, bg, out.m.data_ptr(), ld + 8, stream()) == 0
    torch.cuda.synchronize()
    torch.testing.assert_close(out.m[:, :cols].float(), ref, rtol=8e-3, atol=1e-6)
    out.check(cols)
    if out is not d:
        d.check(0)                                                 # the input is read only
    if mode != "out_of_place_tile":
        torch.testing.assert_close(bias, out.m[:, :cols].float().sum(0), rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------------------------------------------------------ NT GEMM
@pytest.mark.parametrize("M", [128, 130])                          # one full row tile; one full + one partial
@pytest.mark.parametrize("N", [128, 136, 12])                      # full column tile, partial 8-column groups (wide epilogue), N % 8 != 0 (narrow)
@pytest.mark.parametrize("epilogue", ["bias", "elu_bwd"])
def test_gemm_nt_and_pair(lib, M, N, epilogue):
    from go1_gym_learn.ppo_cse import fused
    g = gen(M + N)
    K = 64
    a = bf(torch.randn(M, K, device="cuda", generator=g))
    ws = [bf(torch.randn(N, K, device="cuda", generator=g) / K ** 0.5) for _ in range(2)]
    bias = torch.randn(N, device="cuda", generator=g)
    ldc = N + 8 if N % 8 == 0 else N + 4
    h = bf(F.elu(torch.randn(M, N, device="cuda", generator=g)))
    outs = [Guarded(M, ldc, torch.bfloat16) for _ in range(3)]
    kw = dict(elu_bwd_of=h) if epilogue == "elu_bwd" else dict(bias=bias)
    fused.gemm_nt(lib, a, ws[0], outs[0].m[:, :N], **kw)
    fused.gemm_nt_pair(lib, dict(a=a, b=ws[0], c=outs[1].m[:, :N], **kw), dict(a=a, b=ws[1], c=outs[2].m[:, :N], **kw))
    torch.cuda.synchronize()
    for o, w in zip(outs, (ws[0], ws[0], ws[1])):
        pre = a.float() @ w.float().t() + (0.0 if epilogue == "elu_bwd" else bias)
        ref = pre * elu_prime(h.float()) if epilogue == "elu_bwd" else pre
        err = (o.m[:, :N].float() - ref).abs()
        assert torch.all(err <= 2 ** -8 * (ref.abs() + pre.abs().clamp(min=1.0)) + 1e-6), float(err.max())
        o.check(N)
    assert torch.equal(outs[0].m[:, :N], outs[1].m[:, :N])


# ------------------------------------------------------------------------------------------------------------------ MLP end
@pytest.mark.parametrize("M", [64, 200])
def test_mlp2_forward_and_backward(lib, M):
    from go1_gym_learn.ppo_cse import fused
    g = gen(M)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    fw, bw, keep = (fused.Mlp2Fwd * 2)(), (fused.Mlp2Bwd * 2)(), []
    for i, elu_input in enumerate((1, 0)):
        x = Guarded(M, 264, torch.bfloat16, init=bf(rn(M, 256) * 1.5))
        W2, b2, W3, b3 = bf(rn(128, 256) / 16), bf(rn(128) * 0.1), bf(rn(64, 128) / 11), bf(rn(64) * 0.1)
        z2, out = Guarded(M, 136, torch.bfloat16), Guarded(M, 72, torch.bfloat16)
        d_out = bf(rn(M, 64))
        d_z2, d_x = Guarded(M, 136, torch.bfloat16), Guarded(M, 264, torch.bfloat16)
        x0 = x.m[:, :256].float().clone()
        P, Q = fw[i], bw[i]
        P.x, P.W2, P.b2, P.W3, P.b3, P.z2, P.out = x.m.data_ptr(), W2.data_ptr(), b2.data_ptr(), W3.data_ptr(), b3.data_ptr(), z2.m.data_ptr(), out.m.data_ptr()
        P.rows, P.ld_x, P.ld_z2, P.ld_out, P.elu_input = M, 264, 136, 72, elu_input
        Q.d_out, Q.z2, Q.h, Q.W2, Q.W3, Q.d_z2, Q.d_x = d_out.data_ptr(), z2.m.data_ptr(), x.m.data_ptr(), W2.data_ptr(), W3.data_ptr(), d_z2.m.data_ptr(), d_x.m.data_ptr()
        Q.rows, Q.ld_dout, Q.ld_z2, Q.ld_h, Q.ld_dz2, Q.ld_dx = M, 64, 136, 264, 136, 264
        keep.append((x, x0, W2, b2, W3, b3, z2, out, d_out, d_z2, d_x, elu_input))
    assert lib.go1ppo_mlp2_fwd(fw, 2, stream()) == 0
    assert lib.go1ppo_mlp2_bwd(bw, 2, stream()) == 0
    torch.cuda.synchronize()
    ulp = 2.0 ** -8
    close = lambda a, b, scale: torch.testing.assert_close(a.float(), b, rtol=2 * ulp, atol=2 * ulp * scale)
    for x, x0, W2, b2, W3, b3, z2, out, d_out, d_z2, d_x, elu_input in keep:
        h0 = bf(F.elu(x0)).float() if elu_input else x0
        close(x.m[:, :256], h0, 1.0)
        x.check(256 if elu_input else 0)                           # activated in place, or not written at all
        z2f = z2.m[:, :128].float()
        close(z2.m[:, :128], F.elu(h0 @ W2.float().t() + b2.float()), 1.0)
        z2.check(128)
        close(out.m[:, :64], z2f @ W3.float().t() + b3.float(), 1.0)
        out.check(64)
        dz2_ref = (d_out.float() @ W3.float()) * elu_prime(z2f)
        close(d_z2.m[:, :128], dz2_ref, float(dz2_ref.abs().max()) / 4)
        d_z2.check(128)
        dx_ref = (d_z2.m[:, :128].float() @ W2.float()) * elu_prime(x.m[:, :256].float())
        close(d_x.m[:, :256], dx_ref, float(dx_ref.abs().max()) / 4)
        d_x.check(256)


# ------------------------------------------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize("rows", [128, 192])
def test_batched_weight_gradient_slab_rows(lib, rows):
    """one table: an n = 64, k = 64 problem on the 128-tile (three quarters of the tile are outside the matrix), an n = 256 problem on the
    wide tile with a structural-zero block that starts and ends inside a 16-byte group, a k = 200 problem (last column tile partly
    filled), all three with slabs — and a problem without slabs (fp32 atomics on top of what the buffer holds).  Every slab holds its
    row chunk's product; masked elements, the ldw padding and the bytes around keep their canaries."""
    from go1_gym_learn.ppo_cse import fused
    g = gen(rows)
    #         n,   k, ldw, mask,            slabs
    shapes = [(64, 64, 72, (0, 0, 0), True), (256, 136, 136, (200, 66, 75), True), (72, 200, 208, (9, 1, 6), True), (64, 128, 128, (0, 0, 0), False)]
    tab = (fused.WgradProblem * len(shapes))()
    keep = []
    for P, (n, k, ldw, zero, slabs) in zip(tab, shapes):
        dz, h = bf(torch.randn(rows, n + 8, device="cuda", generator=g)), bf(torch.randn(rows, k + 16, device="cuda", generator=g))
        bias = torch.full((n,), -2.0, device="cuda")
        dW = Guarded(n, ldw, torch.float32, fill=1.0)
        P.dz, P.h, P.dW, P.bias_grad = dz.data_ptr(), h.data_ptr(), dW.m.data_ptr(), bias.data_ptr()
        P.rows, P.ld_dz, P.ld_h, P.n, P.k, P.ldw = rows, n + 8, k + 16, n, k, ldw
        P.zero_n, P.zero_k0, P.zero_k1 = zero
        if slabs:
            P.partials, P.partial_stride = 16, n * ldw             # placeholder: the plan depends on whether a problem has slabs, not where
        keep.append([dz, h, bias, dW, None])
    total = lib.go1ppo_wgrad_tn_plan(tab, len(shapes))
    assert total > 0
    for P, K_, (n, k, ldw, zero, slabs) in zip(tab, keep, shapes):
        if slabs:
            S = -(-P.rows // P.chunk_rows)
            K_[4] = Guarded(S * n, ldw, torch.float32, fill=3.0)
            P.partials, P.partial_stride = K_[4].m.data_ptr(), n * ldw
    assert lib.go1ppo_wgrad_tn_plan(tab, len(shapes)) == total
    dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
    assert lib.go1ppo_wgrad_tn_batched(dev.data_ptr(), len(shapes), total, stream()) == 0
    torch.cuda.synchronize()
    tol = dict(rtol=1e-4, atol=2e-3 * rows ** 0.5)
    for P, (dz, h, bias, dW, slab), (n, k, ldw, zero, slabs) in zip(tab, keep, shapes):
        torch.testing.assert_close(bias, dz[:, :n].float().sum(0) - 2.0, **tol)
        mask = torch.zeros(n, k, dtype=torch.bool, device="cuda")
        mask[:zero[0], zero[1]:zero[2]] = True
        if not slabs:
            torch.testing.assert_close(dW.m[:, :k], dz[:, :n].float().t() @ h[:, :k].float() + 1.0, **tol)
            dW.check(k)
            continue
        dW.check(0)                                                # with slabs the gradient buffer itself is not written
        S = -(-P.rows // P.chunk_rows)
        for s in range(S):
            r0, r1 = s * P.chunk_rows, min(rows, (s + 1) * P.chunk_rows)
            ref = dz[r0:r1, :n].float().t() @ h[r0:r1, :k].float()
            got = slab.m[s * n:(s + 1) * n, :k]
            torch.testing.assert_close(got[~mask], ref[~mask], **tol)
        slab.check(k, row_mask=mask.repeat(S, 1))


def test_weight_gradient_slabs_sum_to_the_product(lib):
    """the slab pieces summed by go1ppo_grad_reduce and by the norm pass (go1ppo_opt_prestep_pieces) — whose sums are written through —
    into a canary-guarded flat gradient: the product with exact zeros on the mask, nothing outside the piece, both passes bit-equal"""
    from go1_gym_learn.ppo_cse import fused
    g = gen(11)
    rows, n, k, off, zero = 192, 256, 136, 1024, (200, 66, 75)
    dz, h = bf(torch.randn(rows, n, device="cuda", generator=g)), bf(torch.randn(rows, k, device="cuda", generator=g))
    flat = Guarded(1, off + n * k + 40, torch.float32, init=torch.randn(1, off + n * k + 40, device="cuda", generator=g))
    plain = flat.m[0].clone()
    tab = (fused.WgradProblem * 1)()
    P = tab[0]
    P.dz, P.h, P.dW, P.bias_grad = dz.data_ptr(), h.data_ptr(), flat.m[0, off:].data_ptr(), None
    P.rows, P.ld_dz, P.ld_h, P.n, P.k, P.ldw = rows, n, k, n, k, k
    P.zero_n, P.zero_k0, P.zero_k1 = zero
    P.partials, P.partial_stride = 16, n * k
    total = lib.go1ppo_wgrad_tn_plan(tab, 1)
    assert total > 0
    S = -(-P.rows // P.chunk_rows)
    ws = torch.zeros(S, n * k, device="cuda")
    P.partials = ws.data_ptr()
    assert lib.go1ppo_wgrad_tn_plan(tab, 1) == total
    arr = (fused.GradPiece * 1)()
    A = arr[0]
    A.begin, A.count, A.src, A.stride, A.kind, A.slabs, A.cols = off, n * k, ws.data_ptr(), n * k, 1, S, k
    A.zero_rows, A.zero_c0, A.zero_c1 = zero
    dev_tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
    dev_pieces = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    ref = dz.float().t() @ h.float()
    ref[:zero[0], zero[1]:zero[2]] = 0
    n_norm = off + n * k + 17
    partial = torch.zeros(lib.go1ppo_opt_partials(), device="cuda")
    step, lr = torch.zeros(1, device="cuda"), torch.full((1,), 1e-3, device="cuda")
    results = []
    for reduce in (lambda: lib.go1ppo_grad_reduce(flat.m.data_ptr(), dev_pieces.data_ptr(), 1, stream()),
                   lambda: lib.go1ppo_opt_prestep_pieces(flat.m.data_ptr(), n_norm, dev_pieces.data_ptr(), 1, 0.5, partial.data_ptr(), step.data_ptr(),
                                                         lr.data_ptr(), None, 1.0, 0.01, 1e-5, 1e-2, stream())):
        flat.m[0].copy_(plain)
        assert lib.go1ppo_wgrad_tn_batched(dev_tab.data_ptr(), 1, total, stream()) == 0
        assert reduce() == 0
        torch.cuda.synchronize()
        got = flat.m[0, off:off + n * k].view(n, k)
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=2e-3 * rows ** 0.5)
        assert bool((got[:zero[0], zero[1]:zero[2]] == 0).all())
        assert torch.equal(flat.m[0, :off], plain[:off]) and torch.equal(flat.m[0, off + n * k:], plain[off + n * k:])
        flat.check(flat.ld)
        results.append(flat.m[0].clone())
    assert torch.equal(results[0], results[1])
    want = float((results[1][:n_norm].double() * 0.5).square().sum())
    assert abs(float(partial.double().sum()) - want) <= 1e-5 * want


# ------------------------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("ranges", [[(0, 4096), (4096, 1920)],     # multiples of 8
                                    [(0, 4100), (4100, 1916)],     # multiples of 4 only
                                    [(0, 4101), (4101, 1915)],     # neither: the one-element path
                                    [(8, 1000), (5000, 1016)]])    # a gap between the ranges; the second crosses n_body
def test_adam_store_paths(lib, ranges):
    """parameters, moments, the bf16 compute copy, the fp32 tail and both transposed copies, on the four-element and the one-element path,
    against torch.optim.Adam over the visited elements; zero_grad clears the visited gradient elements and no other; nothing outside the
    ranges or the buffers changes"""
    from go1_gym_learn.ppo_cse import fused
    g = gen(sum(a + b for a, b in ranges))
    n_body, n_std, n = 6002, 12, 6016
    visited = torch.zeros(n, dtype=torch.bool, device="cuda")
    for a, b in ranges:
        visited[a:a + b] = True
    master = Guarded(1, n, torch.float32, init=torch.randn(1, n, device="cuda", generator=g) * 0.1)
    grad = Guarded(1, n, torch.float32)
    body, std = Guarded(1, n_body, torch.bfloat16), Guarded(1, n_std, torch.float32)
    p = master.m[0]
    p.grad = grad.m[0]
    ref = p.detach().clone().requires_grad_()
    ref_opt = torch.optim.Adam([ref], lr=1e-3)
    opt = fused.FusedAdam(lib, p, body.m[0], std.m[0], n_body, 1e-3, ranges=ranges)
    m, v = Guarded(1, n, torch.float32, fill=0.0), Guarded(1, n, torch.float32, fill=0.0)
    opt.m, opt.v = m.m[0], v.m[0]
    t0, t1 = (16, 16, 48), (5008, 64, 8)                           # (start, rows, cols): one block per range
    d0, d1 = Guarded(t0[2], t0[1], torch.bfloat16, fill=9.0), Guarded(t1[2], t1[1], torch.bfloat16, fill=9.0)
    opt.set_transposes([(t0[0], t0[1], t0[2], d0.m), (t1[0], t1[1], t1[2], d1.m)])
    p0 = p.detach().clone()
    for it in range(3):
        gr = torch.randn(n, device="cuda", generator=g)
        grad.m[0].copy_(gr)
        opt.step_(zero_grad=True)
        ref.grad = torch.where(visited, gr, torch.zeros_like(gr))
        ref_opt.step()
        torch.cuda.synchronize()
        assert bool((grad.m[0][visited] == 0).all()) and torch.equal(grad.m[0][~visited], gr[~visited])
        torch.testing.assert_close(p.detach()[visited], ref.detach()[visited], rtol=2e-5, atol=2e-7)
        assert torch.equal(p.detach()[~visited], p0[~visited])
    for buf in (master, grad, m, v):
        buf.check(n)
    assert not m.m[0][~visited].any() and not v.m[0][~visited].any()
    vb = visited[:n_body]
    assert torch.equal(body.m[0][vb], bf(p.detach()[:n_body])[vb])
    body.check(n_body, row_mask=(~vb)[None])
    vs = visited[n_body:n_body + n_std]
    assert torch.equal(std.m[0][vs], p.detach()[n_body:n_body + n_std][vs])
    std.check(n_std, row_mask=(~vs)[None])
    for (st, r, c), d in ((t0, d0), (t1, d1)):
        inb = (visited[st:st + r * c] & (torch.arange(st, st + r * c, device="cuda") < n_body)).view(r, c).t()
        want = bf(p.detach()[st:st + r * c]).view(r, c).t()
        assert torch.equal(d.m[inb], want[inb])
        d.check(r, row_mask=~inb)


# ------------------------------------------------------------------------------------------------------------------ ring gather
def test_ring_gather_rows(lib):
    g = gen(5)
    N, T, H, no, npv = 2, 3, 4, 6, 2
    Kp = H * no + 1 + npv + 5                                      # [window | 1 | privileged | zero padding]
    ring = bf(torch.randn(T + H - 1, N, no, device="cuda", generator=g))
    priv = torch.randn(T * N, npv, device="cuda", generator=g)
    idx = torch.tensor([5, 0, 3, 4, 1, 2], device="cuda", dtype=torch.int64)
    X = Guarded(idx.numel(), Kp, torch.bfloat16)
    assert lib.go1ppo_ring_gather(ring.data_ptr(), priv.data_ptr(), idx.data_ptr(), idx.numel(), N, H, no, npv, Kp, X.m.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    for i, f in enumerate(idx.tolist()):
        s, e = divmod(f, N)
        want = torch.cat([ring[s:s + H, e].reshape(-1).float(), torch.ones(1, device="cuda"), bf(priv[f]).float(), torch.zeros(5, device="cuda")])
        assert torch.equal(X.m[i].float(), want), i
    X.check(Kp)


# ------------------------------------------------------------------------------------------------------------------ visibility
def test_written_through_outputs_are_visible_to_the_next_launch(lib):
    """a producer whose output is written through (the in-place ELU) and its consumer (the NT GEMM reading that output): back to back on
    one stream, and across two streams joined by an event, against the run with a device synchronisation between the two launches"""
    from go1_gym_learn.ppo_cse import fused
    g = gen(9)
    M, K, N = 1000, 256, 136
    x0 = bf(torch.randn(M, K, device="cuda", generator=g) * 2)
    w = bf(torch.randn(N, K, device="cuda", generator=g) / 16)
    bias = torch.randn(N, device="cuda", generator=g)

    def run(mode):
        x, c = x0.clone(), torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
        torch.cuda.synchronize()
        if mode == "two_streams":
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            with torch.cuda.stream(s1):
                assert lib.go1ppo_elu_fwd(x.data_ptr(), M, K, K, None, 0, 0, None, 0, 0, stream()) == 0
                ev = s1.record_event()
            with torch.cuda.stream(s2):
                s2.wait_event(ev)
                fused.gemm_nt(lib, x, w, c, bias)
        else:
            assert lib.go1ppo_elu_fwd(x.data_ptr(), M, K, K, None, 0, 0, None, 0, 0, stream()) == 0
            if mode == "synchronised":
                torch.cuda.synchronize()
            fused.gemm_nt(lib, x, w, c, bias)
        torch.cuda.synchronize()
        return x, c
    xr, cr = run("synchronised")
    torch.testing.assert_close(xr.float(), bf(F.elu(x0.float())).float(), rtol=8e-3, atol=1e-6)
    for mode in ("one_stream", "two_streams"):
        x, c = run(mode)
        assert torch.equal(x, xr) and torch.equal(c, cr), mode
