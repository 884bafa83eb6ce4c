"""Kernel numerics on the GPU: every HIP kernel against a plain PyTorch fp32 reference of the same op (computed on
bf16-rounded operands where the kernel consumes bf16).  All calls go through the C ABI (vit_amd.functional -> ctypes)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-20))


def bf(t):
    return t.to(torch.bfloat16)


def randn(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


GEMM_SHAPES = [(128, 128, 64), (320, 192, 192), (104, 40, 72), (516, 96, 32), (2064, 768, 768), (256, 3072, 768), (640, 768, 3072)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("layout", ["nt", "nn", "tn", "tt"])
def test_gemm_layouts(dev, M, N, K, layout):
    import vit_amd.functional as vf

    # nt: A [M,K], B [N,K] (forward) | nn: B stored [K,N] (dX) | tn: A stored [K,M], B stored [K,N] (dW) | tt: A [K,M], B [N,K]
    a_t = layout in ("tn", "tt")
    b_t = layout in ("nn", "tn")
    A = bf(randn((M, K), dev, 1))
    Bm = bf(randn((N, K), dev, 2))
    ref = A.float() @ Bm.float().t()
    a_store = A.t().contiguous() if a_t else A
    b_store = Bm.t().contiguous() if b_t else Bm
    if a_t and M % 8:
        pytest.skip("transposed A needs M % 8 == 0")
    out = vf.gemm(a_store, b_store, M=M, N=N, K=K, a_trans=a_t, b_trans=b_t, out_dtype=torch.float32)
    assert rel(out, ref) < 2e-5, (layout, rel(out, ref))
    out16 = vf.gemm(a_store, b_store, M=M, N=N, K=K, a_trans=a_t, b_trans=b_t, out_dtype=torch.bfloat16)
    assert rel(out16, ref) < 4e-3


def test_gemm_identity_asymmetric(dev):
    """A = I with an asymmetric B catches swapped row/col maps (CDNA guide, section 3)."""
    import vit_amd.functional as vf

    n = 128
    A = bf(torch.eye(n, device=dev))
    Bm = bf(torch.arange(n * n, device=dev, dtype=torch.float32).reshape(n, n) % 251)
    out = vf.gemm(A, Bm, M=n, N=n, K=n, out_dtype=torch.float32)
    assert torch.equal(out, Bm.float().t().contiguous())
    out = vf.gemm(A, Bm, M=n, N=n, K=n, b_trans=True, out_dtype=torch.float32)
    assert torch.equal(out, Bm.float())
    out = vf.gemm(Bm, A, M=n, N=n, K=n, a_trans=True, out_dtype=torch.float32)
    assert torch.equal(out, Bm.float().t().contiguous())


def test_gemm_epilogues(dev):
    import vit_amd.functional as vf
    from vit_amd._cabi import ACT_DGELU, ACT_GELU

    M, N, K = 330, 256, 192
    x, W = bf(randn((M, K), dev, 3)), bf(randn((N, K), dev, 4, 0.1))
    bias = randn((N,), dev, 5)
    res = randn((M, N), dev, 6)
    base = x.float() @ W.float().t() + bias
    # bias + GELU + saved pre-activation
    aux = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    y = vf.linear_fwd(x, W, bias, act=ACT_GELU, aux_out=aux)
    assert rel(aux, base) < 4e-3
    assert rel(y, F.gelu(base)) < 5e-3
    # bias + residual, f32 out
    y = vf.linear_fwd(x, W, bias, out_dtype=torch.float32, residual=res)
    assert rel(y, base + res) < 2e-5
    # dX with dgelu
    dy = bf(randn((M, N), dev, 7))
    u = bf(randn((M, K), dev, 8))
    dx = vf.linear_bwd_dx(dy, W, dgelu_aux=u, out_dtype=torch.float32)
    uu = u.float().requires_grad_(True)
    F.gelu(uu).backward(dy.float() @ W.float())
    assert rel(dx, uu.grad) < 2e-5
    # dW (split-K over M) and accumulate
    dw = vf.linear_bwd_dw(dy, x)
    refdw = dy.float().t() @ x.float()
    assert rel(dw, refdw) < 2e-5
    dw2 = vf.linear_bwd_dw(dy, x, out=dw.clone(), accumulate=True)
    assert rel(dw2, 2 * refdw) < 2e-5
    # row map: rows b*rpb + n -> b*orb + n + 1
    Bn, rpb = 6, 55
    xx = bf(randn((Bn * rpb, K), dev, 9))
    out = torch.full((Bn * (rpb + 1), N), 7.0, dtype=torch.float32, device=dev)
    vf.gemm(xx, W, M=Bn * rpb, N=N, K=K, out=out, bias=bias, row_map=(rpb, rpb + 1, 1))
    ref = (xx.float() @ W.float().t() + bias).view(Bn, rpb, N)
    o3 = out.view(Bn, rpb + 1, N)
    assert rel(o3[:, 1:], ref) < 2e-5
    assert torch.all(o3[:, 0] == 7.0)


def test_gemm_split_k_explicit(dev):
    import vit_amd.functional as vf

    M, N, K = 96, 64, 4096
    a, b = bf(randn((M, K), dev, 10)), bf(randn((N, K), dev, 11))
    ref = a.float() @ b.float().t()
    for sk in (2, 5, 64):
        out = vf.gemm(a, b, M=M, N=N, K=K, out_dtype=torch.float32, split_k=sk)
        assert rel(out, ref) < 2e-5
    # determinism: bitwise equal across runs
    o1 = vf.gemm(a, b, M=M, N=N, K=K, out_dtype=torch.float32, split_k=8)
    o2 = vf.gemm(a, b, M=M, N=N, K=K, out_dtype=torch.float32, split_k=8)
    assert torch.equal(o1, o2)


def test_gemm_dropout_mask_consistency(dev):
    import vit_amd.functional as vf

    M, N, K = 512, 384, 64
    x = bf(torch.zeros((M, K), device=dev))
    W = bf(torch.zeros((N, K), device=dev))
    ones = torch.ones((N,), device=dev)
    drop = (0.1, 1234, 7)
    y = vf.linear_fwd(x, W, ones, out_dtype=torch.float32, dropout=drop)   # = mask * scale
    keep = (y != 0).float().mean().item()
    assert abs(keep - 0.9) < 0.01
    scale = y.max().item()
    assert abs(scale - 1 / 0.9) < 1e-3
    dy = vf.dropout_bwd_cast(torch.ones((M, N), device=dev), drop)
    assert torch.equal(dy.float() != 0, y != 0)
    # another site / seed gives another mask
    y2 = vf.linear_fwd(x, W, ones, out_dtype=torch.float32, dropout=(0.1, 1234, 8))
    assert not torch.equal(y2 != 0, y != 0)
    # columns and rows are not correlated
    m = (y != 0).float()
    assert abs(m.mean(0).std().item()) < 0.03 and abs(m.mean(1).std().item()) < 0.03


@pytest.mark.parametrize("rows,D", [(516, 32), (320, 192), (1000, 768), (77, 1024), (33, 2048)])
def test_layernorm(dev, rows, D):
    import vit_amd.functional as vf

    x = randn((rows, D), dev, 20) * 3 + 0.5
    g, b = randn((D,), dev, 21) * 0.1 + 1, randn((D,), dev, 22) * 0.1
    eps = 1e-12
    y32, mean, rstd = vf.layernorm_fwd(x, g, b, eps, out_dtype=torch.float32)
    ref = F.layer_norm(x, (D,), g, b, eps)
    assert rel(y32, ref) < 1e-6
    assert rel(mean, x.mean(-1)) < 1e-6
    y16, _, _ = vf.layernorm_fwd(x, g, b, eps, out_dtype=torch.bfloat16)
    assert rel(y16, ref) < 4e-3
    # backward
    dy = randn((rows, D), dev, 23)
    dres = randn((rows, D), dev, 24)
    xx = x.clone().requires_grad_(True)
    gg, bb = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    F.layer_norm(xx, (D,), gg, bb, eps).backward(dy)
    dx, dg, db = vf.layernorm_bwd(dy, x, g, mean, rstd, dres=dres)
    assert rel(dx, xx.grad + dres) < 1e-5
    assert rel(dg, gg.grad) < 1e-5 and rel(db, bb.grad) < 1e-5
    dx16, dg16, _ = vf.layernorm_bwd(bf(dy), x, g, mean, rstd)
    xx.grad = None
    gg.grad = None
    F.layer_norm(xx, (D,), gg, bb, eps).backward(bf(dy).float())
    assert rel(dx16, xx.grad) < 1e-5 and rel(dg16, gg.grad) < 1e-5


def attn_ref(qkv, B, H, T, dh, scale, mask=None):
    q, k, v = qkv.float().view(B, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    p = s.softmax(-1)
    pd = p if mask is None else p * mask
    ctx = (pd @ v).permute(0, 2, 1, 3).reshape(B * T, H * dh)
    return ctx, p, torch.logsumexp(s, -1)


# T mod 64 = 1, 5, 44, 0, 26, 56: the resident forward runs its last key tile in a body for 1, 3, (none), 2, 4 sixteen-key blocks
ATT_SHAPES = [(2, 2, 129, 16), (2, 3, 5, 64), (2, 4, 197, 64), (1, 2, 300, 32), (1, 1, 70, 128), (1, 2, 64, 64), (1, 2, 90, 64),
              (1, 2, 120, 32), (1, 1, 577, 64),
              (1, 2, 1025, 16), (1, 1, 640, 64),  # these two: past the resident kernels
              (1, 2, 4034, 16), (1, 1, 4034, 64),  # the stride sweep's longest sequences (configs/sweep.yaml: S = 1 at L = 4096, P = 64)
              (2, 12, 197, 64), (1, 12, 193, 64), (1, 12, 208, 64), (23, 12, 197, 64),  # 12 heads, 192 < T <= 208: the compile-time forms
              (1, 16, 577, 64), (2, 16, 592, 64),  # the ViT-L head count and sequence
              # head sizes that are multiples of 4 but not of 8 (heads at 8-byte offsets; configs/sweep.yaml reaches hidden 32 /
              # 8 heads = 4): short, one tile, and the sweep's longest sequence
              (2, 8, 122, 4), (1, 8, 64, 4), (1, 8, 4090, 4), (2, 3, 130, 12), (1, 2, 77, 20)]


@pytest.mark.parametrize("B,H,T,dh", ATT_SHAPES)
def test_attention_fwd_bwd(dev, B, H, T, dh):
    import vit_amd.functional as vf

    scale = dh ** -0.5
    qkv = bf(randn((B * T, 3 * H * dh), dev, 30))
    ctx, lse = vf.attention_fwd(qkv, B, H, T, dh, scale)
    q32 = qkv.float().requires_grad_(True)
    ref, p, lse_ref = attn_ref(q32, B, H, T, dh, scale)
    assert rel(ctx, ref) < 6e-3
    assert rel(lse, lse_ref.reshape(B * H, T)) < 1e-5
    probs = vf.attention_probs(qkv, B, H, T, dh, scale)
    assert rel(probs, p) < 1e-5
    dctx = bf(randn((B * T, H * dh), dev, 31))
    ref.backward(dctx.float())
    dqkv = vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, scale)
    g = q32.grad.view(B * T, 3, H * dh)
    d = dqkv.float().view(B * T, 3, H * dh)
    for i, nm in enumerate("qkv"):
        assert rel(d[:, i], g[:, i]) < 1.5e-2, (nm, rel(d[:, i], g[:, i]))


def extract_attn_mask(vf, dev, B, H, T, dh, drop):
    """Recover the dropout multiplier M[b,h,q,k] of the attention kernel: with Q=K=0 the probabilities are 1/T, and a
    one-hot V block makes ctx[q, d] = M[q, i*dh+d] / T."""
    mask = torch.zeros((B, H, T, T), device=dev)
    for i in range(math.ceil(T / dh)):
        qkv = torch.zeros((B, T, 3, H, dh), device=dev)
        for d in range(dh):
            k = i * dh + d
            if k < T:
                qkv[:, k, 2, :, d] = 1.0
        ctx, _ = vf.attention_fwd(bf(qkv.view(B * T, 3 * H * dh)), B, H, T, dh, 1.0, dropout=drop)
        c = ctx.float().view(B, T, H, dh).permute(0, 2, 1, 3) * T   # [B,H,T(q),dh]
        n = min(dh, T - i * dh)
        mask[:, :, :, i * dh:i * dh + n] = c[..., :n]
    return mask


@pytest.mark.parametrize("B,H,T,dh", [(2, 2, 129, 16), (1, 3, 197, 64), (1, 12, 197, 64), (2, 8, 122, 4), (1, 2, 700, 12)])
def test_attention_dropout(dev, B, H, T, dh):
    import vit_amd.functional as vf

    drop = (0.1, 99, 3)
    scale = dh ** -0.5
    mask = extract_attn_mask(vf, dev, B, H, T, dh, drop)
    vals = torch.unique(mask.round(decimals=2))
    assert vals.numel() == 2 and abs(vals[1].item() - 1 / 0.9) < 2e-2, vals
    mask = (mask > 0.5).float() * (65536.0 / (65536 - 6554))
    assert abs((mask > 0).float().mean().item() - 0.9) < 0.01
    qkv = bf(randn((B * T, 3 * H * dh), dev, 32))
    ctx, lse = vf.attention_fwd(qkv, B, H, T, dh, scale, dropout=drop)
    q32 = qkv.float().requires_grad_(True)
    ref, _, _ = attn_ref(q32, B, H, T, dh, scale, mask)
    assert rel(ctx, ref) < 6e-3
    dctx = bf(randn((B * T, H * dh), dev, 33))
    ref.backward(dctx.float())
    dqkv = vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, scale, dropout=drop)
    g = q32.grad.view(B * T, 3, H * dh)
    d = dqkv.float().view(B * T, 3, H * dh)
    for i in range(3):
        assert rel(d[:, i], g[:, i]) < 1.5e-2, (i, rel(d[:, i], g[:, i]))


def test_unfold_and_embed(dev):
    import vit_amd.functional as vf

    B, L, P, S = 3, 1000, 64, 48
    N = math.ceil((L - P) / S) + 1
    x = randn((B, L), dev, 40)
    patches = vf.unfold_cast(x, P, S, N)
    ref = x.unfold(1, P, S)
    ref = torch.cat([ref, torch.zeros(B, N - ref.size(1), P, device=dev)], 1).reshape(B * N, P)
    # the reference zero-pads a whole missing patch; a partially covered tail does not occur with unfold semantics
    assert torch.equal(patches.float(), bf(ref).float())
    D, T = 64, N + 1
    tok = randn((B, T, D), dev, 41)
    cls, pos = randn((D,), dev, 42), randn((T, D), dev, 43)
    out = vf.embed_finish(tok.clone(), cls, pos)
    exp = tok.clone()
    exp[:, 0] = cls
    exp = exp + pos
    assert rel(out, exp) < 1e-7
    drop = (0.1, 5, 1)
    outd = vf.embed_finish(tok.clone(), cls, pos, dropout=drop)
    m = (outd != 0).float()
    assert abs(m.mean().item() - 0.9) < 0.02
    assert rel(outd, exp * m * (65536.0 / (65536 - 6554))) < 1e-6
    # backward
    dtok = randn((B, T, D), dev, 44)
    dcls = torch.empty(D, device=dev)
    dpos = torch.empty((T, D), device=dev)
    dpatch = vf.embed_finish_bwd(dtok, dcls, dpos, dropout=drop)
    gm = dtok * m * (65536.0 / (65536 - 6554))
    assert rel(dcls, gm[:, 0].sum(0)) < 1e-6
    assert rel(dpos, gm.sum(0)) < 1e-6
    assert rel(dpatch, gm[:, 1:].reshape(B * N, D)) < 4e-3


def test_colsum_cast_dropout_bwd(dev):
    import vit_amd.functional as vf

    a = randn((1234, 768), dev, 50)
    assert rel(vf.colsum(a), a.sum(0)) < 1e-5
    a16 = bf(a)
    assert rel(vf.colsum(a16), a16.float().sum(0)) < 1e-5
    out = vf.colsum(a16, out=torch.ones(768, device=dev), accumulate=True)
    assert rel(out, a16.float().sum(0) + 1) < 1e-5
    assert torch.equal(vf.cast_f32_bf16(a), a16)
    odd = randn((1003,), dev, 51)
    assert torch.equal(vf.cast_f32_bf16(odd), bf(odd))
    dy = vf.dropout_bwd_cast(a, (0.0, 0, 0))
    assert torch.equal(dy, a16)


@pytest.mark.parametrize("kind,C", [("mse", 1), ("l1", 3), ("ce", 5)])
def test_head_loss(dev, kind, C):
    import vit_amd.functional as vf
    from vit_amd._cabi import LOSS_CE, LOSS_L1, LOSS_MSE

    B, T, D = 37, 6, 192
    last = randn((B, T, D), dev, 60)
    W, b = randn((C, D), dev, 61, 0.1), randn((C,), dev, 62, 0.1)
    if kind == "ce":
        labels = torch.randint(0, C, (B,), device=dev)
        code = LOSS_CE
    else:
        labels = torch.rand((B, C) if C > 1 else (B,), device=dev)
        code = LOSS_L1 if kind == "l1" else LOSS_MSE
    logits, loss = vf.head_loss_fwd(last, W, b, labels, code)
    l32 = last.clone().requires_grad_(True)
    W32, b32 = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lg = F.linear(l32[:, 0], W32, b32)
    if kind == "ce":
        ref = F.cross_entropy(lg, labels)
    elif kind == "l1":
        ref = F.l1_loss(lg.view(-1), labels.view(-1))
    else:
        ref = F.mse_loss(lg.view(-1), labels.view(-1))
    assert rel(logits, lg) < 1e-5 and abs(loss.item() - ref.item()) < 1e-5 * max(1, abs(ref.item()))
    (ref * 1.7).backward()
    dloss = torch.full((1,), 1.7, device=dev)
    dlast, dW, db = vf.head_loss_bwd(last, W, logits, labels, dloss, code)
    assert rel(dlast, l32.grad) < 1e-5 and rel(dW, W32.grad) < 1e-5 and rel(db, b32.grad) < 1e-5


def test_sqnorm_adamw(dev):
    import vit_amd.functional as vf

    n = 1_000_003
    p0, g = randn((n,), dev, 70), randn((n,), dev, 71, 0.01)
    sq = vf.grad_sqnorm(g)
    assert abs(sq.item() - float((g.double() ** 2).sum())) < 1e-4 * sq.item()
    # against torch.optim.AdamW with clip_grad_norm_(0.5)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=1e-3, weight_decay=0.01)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    pb = torch.empty(n, dtype=torch.bfloat16, device=dev)
    for step in range(1, 4):
        gs = g * step
        pt.grad = gs.clone()
        torch.nn.utils.clip_grad_norm_([pt], 0.5)
        opt.step()
        sq = vf.grad_sqnorm(gs)
        vf.adamw_step(p, gs, m, v, pb, lr=1e-3, weight_decay=0.01, step=step, sqnorm=sq, max_norm=0.5)
        assert rel(p, pt.detach()) < 1e-6
    assert torch.equal(pb, bf(p))


# ------------------------------------------------------------------ the LDS-DMA / persistent GEMM core (gemm2.hip)
# (256, 256, 64) / (512, 512, 192): one and three K-tiles -- the ping-pong core's stream cursor runs past the end of the walk
# (clamped re-fetches) from its prologue on
ALIGNED = [(256, 128, 64), (256, 256, 64), (512, 256, 128), (512, 512, 192), (1024, 768, 768), (2304, 768, 256), (768, 3072, 768),
           (1792, 2304, 768)]


@pytest.mark.parametrize("core", [5])
@pytest.mark.parametrize("M,N,K", ALIGNED)
@pytest.mark.parametrize("layout", ["nt", "nn", "tn", "tt"])
def test_gemm2_layouts(dev, core, M, N, K, layout):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    a_t, b_t = layout in ("tn", "tt"), layout in ("nn", "tn")
    A, Bm = bf(randn((M, K), dev, 1)), bf(randn((N, K), dev, 2))
    ref = A.float() @ Bm.float().t()
    a_store = A.t().contiguous() if a_t else A
    b_store = Bm.t().contiguous() if b_t else Bm
    _cabi.set_option("gemm_core", core)
    try:
        out = vf.gemm(a_store, b_store, M=M, N=N, K=K, a_trans=a_t, b_trans=b_t, out_dtype=torch.float32)
        out16 = vf.gemm(a_store, b_store, M=M, N=N, K=K, a_trans=a_t, b_trans=b_t, out_dtype=torch.bfloat16)
        sk = vf.gemm(a_store, b_store, M=M, N=N, K=K, a_trans=a_t, b_trans=b_t, out_dtype=torch.float32, split_k=-1)
    finally:
        _cabi.set_option("gemm_core", 1)
    assert rel(out, ref) < 2e-5, (layout, rel(out, ref))
    assert rel(out16, ref) < 4e-3
    assert rel(sk, ref) < 2e-5


@pytest.mark.parametrize("core", [0, 5])
def test_gemm2_epilogues_match_generic_core(dev, core):
    """Every fused epilogue on a tile-aligned problem, each core against the torch reference (and so against each other)."""
    import vit_amd.functional as vf
    from vit_amd import _cabi
    from vit_amd._cabi import ACT_GELU

    M, N, K = 1024, 768, 512
    x, W = bf(randn((M, K), dev, 3)), bf(randn((N, K), dev, 4, 0.1))
    bias, res = randn((N,), dev, 5), randn((M, N), dev, 6)
    base = x.float() @ W.float().t() + bias
    _cabi.set_option("gemm_core", core)
    try:
        aux = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        y = vf.linear_fwd(x, W, bias, act=ACT_GELU, aux_out=aux)
        assert rel(aux, base) < 4e-3 and rel(y, F.gelu(base)) < 5e-3
        y = vf.linear_fwd(x, W, bias, out_dtype=torch.float32, residual=res)
        assert rel(y, base + res) < 2e-5
        drop = (0.1, 77, 5)
        yd = vf.linear_fwd(x, W, bias, out_dtype=torch.float32, dropout=drop, residual=res)
        mask = vf.dropout_bwd_cast(torch.ones((M, N), device=dev), drop).float()
        assert rel(yd, base * mask + res) < 5e-3  # mask scale is bf16-rounded in this reconstruction
        assert torch.equal((yd - res).abs() > 1e-6, mask != 0) or ((yd - res != 0) == (mask != 0)).float().mean() > 0.999
        dy, u = bf(randn((M, N), dev, 7)), bf(randn((M, K), dev, 8))
        dx = vf.linear_bwd_dx(dy, W, dgelu_aux=u, out_dtype=torch.float32)
        uu = u.float().requires_grad_(True)
        F.gelu(uu).backward(dy.float() @ W.float())
        assert rel(dx, uu.grad) < 2e-5
        dw = vf.linear_bwd_dw(dy, x)
        assert rel(dw, dy.float().t() @ x.float()) < 2e-5
        dw2 = vf.linear_bwd_dw(dy, x, out=dw.clone(), accumulate=True)
        assert rel(dw2, 2 * (dy.float().t() @ x.float())) < 2e-5
        # patch-embed shaped row map: M = B * N rows -> rows 1..N of each sample
        Bn, rpb = 8, 96   # 768 rows
        xx = bf(randn((Bn * rpb, K), dev, 9))
        out = torch.full((Bn * (rpb + 1), N), 7.0, dtype=torch.float32, device=dev)
        vf.gemm(xx, W, M=Bn * rpb, N=N, K=K, out=out, bias=bias, row_map=(rpb, rpb + 1, 1))
        ref = (xx.float() @ W.float().t() + bias).view(Bn, rpb, N)
        o3 = out.view(Bn, rpb + 1, N)
        assert rel(o3[:, 1:], ref) < 2e-5 and torch.all(o3[:, 0] == 7.0)
    finally:
        _cabi.set_option("gemm_core", 1)


def test_gemm2_many_tiles_persistent(dev):
    """More tiles than CUs (several persistent rounds, partial last round) and bitwise run-to-run determinism."""
    import vit_amd.functional as vf

    M, N, K = 256 * 37, 768, 256   # 111 or 222 tiles
    a, b = bf(randn((M, K), dev, 12)), bf(randn((N, K), dev, 13))
    ref = a.float() @ b.float().t()
    o1 = vf.gemm(a, b, M=M, N=N, K=K, out_dtype=torch.float32)
    o2 = vf.gemm(a, b, M=M, N=N, K=K, out_dtype=torch.float32)
    assert rel(o1, ref) < 2e-5 and torch.equal(o1, o2)
    M = 256 * 300                    # 900 / 1800 tiles: > 3 rounds on 256 CUs
    a = bf(randn((M, K), dev, 14))
    o = vf.gemm(a, b, M=M, N=N, K=K, out_dtype=torch.float32)
    assert rel(o, a.float() @ b.float().t()) < 2e-5


@pytest.mark.parametrize("rows,D", [(516, 32), (1000, 768), (77, 1024)])
def test_layernorm_bwd_fused(dev, rows, D):
    """The fused form must equal layernorm_bwd -> dropout_bwd_cast -> colsum on the same inputs (bit for bit on dyn)."""
    import vit_amd.functional as vf

    x = randn((rows, D), dev, 80) * 2 + 0.3
    g, b = randn((D,), dev, 81) * 0.1 + 1, randn((D,), dev, 82) * 0.1
    _, mean, rstd = vf.layernorm_fwd(x, g, b, 1e-12, out_dtype=torch.float32)
    dy, dres = bf(randn((rows, D), dev, 83)), randn((rows, D), dev, 84)
    for drop in ((0.0, 0, 0), (0.1, 321, 9)):
        dx0, dg0, db0 = vf.layernorm_bwd(dy, x, g, mean, rstd, dres=dres)
        dyn0 = vf.dropout_bwd_cast(dx0, drop)
        dbias0 = vf.colsum(dyn0)
        E = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)
        dx1, dg1, db1, dyn1, dbias1 = vf.layernorm_bwd_fused(dy, x, g, mean, rstd, dres, E(rows, D), E(D), E(D),
                                                             E(rows, D, dt=torch.bfloat16), E(D), drop)
        assert torch.equal(dx1, dx0) and torch.equal(dyn1, dyn0)
        assert rel(dg1, dg0) < 1e-6 and rel(db1, db0) < 1e-6 and rel(dbias1, dbias0) < 1e-5


@pytest.mark.parametrize("rows,D", [(37, 32), (1000, 192), (3940, 768), (129, 1024)])
@pytest.mark.parametrize("ddt", [torch.bfloat16, torch.float32])
def test_layernorm_fwd_residual(dev, rows, D, ddt):
    """LayerNorm over x + delta with the sum written back (the residual add of ViTLayer / ViTOutput): the sum is exact,
    statistics and output equal the plain kernel's on the summed rows bit for bit."""
    import vit_amd.functional as vf

    x = randn((rows, D), dev, 90) * 2 + 0.3
    delta = (randn((rows, D), dev, 91)).to(ddt)
    g, b = randn((D,), dev, 92) * 0.1 + 1, randn((D,), dev, 93) * 0.1
    xs = torch.empty_like(x)
    for odt in (torch.bfloat16, torch.float32):
        y, mean, rstd = vf.layernorm_fwd_residual(x, delta, xs, g, b, 1e-12, out_dtype=odt)
        ref_sum = x + delta.float()
        assert torch.equal(xs, ref_sum)
        y0, mean0, rstd0 = vf.layernorm_fwd(ref_sum, g, b, 1e-12, out_dtype=odt)
        assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)


# ------------------------------------------------------------------ fp32-class kernels (precision='32')
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (320, 192, 192), (104, 40, 72), (516, 96, 32), (1024, 768, 768)])
@pytest.mark.parametrize("layout", ["nt", "nn", "tn", "tt"])
def test_gemm_x3_f32_operands(dev, M, N, K, layout):
    """Split-bf16 x3 GEMM on f32 operands against an fp64 reference: ~1e-5 relative."""
    import vit_amd.functional as vf

    a_t, b_t = layout in ("tn", "tt"), layout in ("nn", "tn")
    if a_t and M % 8:
        pytest.skip("transposed A needs M % 8 == 0")
    A, Bm = randn((M, K), dev, 1), randn((N, K), dev, 2)
    ref = (A.double() @ Bm.double().t()).float()
    a_store = A.t().contiguous() if a_t else A
    b_store = Bm.t().contiguous() if b_t else Bm
    out = vf.gemm(a_store, b_store, M=M, N=N, K=K, a_trans=a_t, b_trans=b_t, out_dtype=torch.float32)
    assert rel(out, ref) < 3e-5, (layout, rel(out, ref))
    sk = vf.gemm(a_store, b_store, M=M, N=N, K=K, a_trans=a_t, b_trans=b_t, out_dtype=torch.float32, split_k=-1)
    assert rel(sk, ref) < 3e-5


def test_gemm_x3_epilogues(dev):
    import vit_amd.functional as vf
    from vit_amd._cabi import ACT_GELU

    M, N, K = 330, 256, 192
    x, W = randn((M, K), dev, 3), randn((N, K), dev, 4, 0.1)
    bias, res = randn((N,), dev, 5), randn((M, N), dev, 6)
    base = (x.double() @ W.double().t()).float() + bias
    aux = torch.empty((M, N), dtype=torch.float32, device=dev)
    y = vf.linear_fwd(x, W, bias, out_dtype=torch.float32, act=ACT_GELU, aux_out=aux)
    assert rel(aux, base) < 3e-5 and rel(y, F.gelu(base)) < 3e-5
    y = vf.linear_fwd(x, W, bias, out_dtype=torch.float32, residual=res)
    assert rel(y, base + res) < 3e-5
    dy, u = randn((M, N), dev, 7), randn((M, K), dev, 8)
    dx = vf.linear_bwd_dx(dy, W, dgelu_aux=u, out_dtype=torch.float32)
    uu = u.clone().requires_grad_(True)
    F.gelu(uu).backward((dy.double() @ W.double()).float())
    assert rel(dx, uu.grad) < 3e-5
    dw = vf.linear_bwd_dw(dy, x)
    assert rel(dw, (dy.double().t() @ x.double()).float()) < 3e-5


@pytest.mark.parametrize("B,H,T,dh", [(2, 2, 129, 16), (2, 3, 5, 64), (1, 2, 197, 64), (1, 1, 70, 128), (2, 2, 130, 64),
                                      (1, 2, 577, 64), (3, 1, 64, 64), (2, 8, 122, 4), (1, 8, 1030, 4), (1, 3, 130, 12)])  # head_dim 64: the f32-MFMA kernels; others: one wave per row
def test_attention_f32(dev, B, H, T, dh):
    import vit_amd.functional as vf

    scale = dh ** -0.5
    qkv = randn((B * T, 3 * H * dh), dev, 30)
    ctx, lse = vf.attention_fwd(qkv, B, H, T, dh, scale)
    q32 = qkv.clone().requires_grad_(True)
    ref, p, lse_ref = attn_ref(q32, B, H, T, dh, scale)
    assert rel(ctx, ref) < 1e-5 and rel(lse, lse_ref.reshape(B * H, T)) < 1e-6
    assert rel(vf.attention_probs(qkv, B, H, T, dh, scale), p) < 1e-5
    dctx = randn((B * T, H * dh), dev, 31)
    ref.backward(dctx)
    dqkv = vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, scale)
    assert rel(dqkv, q32.grad) < 2e-5
    # dropout: same mask function as the bf16 kernels (row = bh*T + q, column pair = key / 2)
    drop = (0.1, 99, 3)
    mask = extract_attn_mask(vf, dev, B, H, T, dh, drop) if dh <= 64 else None
    if mask is not None:
        mask = (mask > 0.5).float() * (65536.0 / (65536 - 6554))
        ctxd, lsed = vf.attention_fwd(qkv, B, H, T, dh, scale, dropout=drop)
        q32 = qkv.clone().requires_grad_(True)
        refd, _, _ = attn_ref(q32, B, H, T, dh, scale, mask)
        assert rel(ctxd, refd) < 1e-5
        refd.backward(dctx)
        assert rel(vf.attention_bwd(qkv, ctxd, dctx, lsed, B, H, T, dh, scale, dropout=drop), q32.grad) < 2e-5


def test_add_noise_distribution(dev):
    """vit_add_noise (vit.py:86-88): out - flux = z * error * level with z ~ N(0,1): moments, tails, independence of the
    launch geometry (same seed -> same noise), different seeds decorrelated."""
    import vit_amd.functional as vf

    n = 1 << 22
    flux, err = randn((n,), dev, 100), torch.rand(n, device=dev) * 0.2 + 0.05
    out = vf.add_noise(flux, err, 0.5, seed=1234)
    z = ((out - flux) / (err * 0.5)).double()
    assert abs(float(z.mean())) < 3e-3 and abs(float(z.var()) - 1.0) < 5e-3
    assert abs(float((z ** 3).mean())) < 2e-2 and abs(float((z ** 4).mean()) - 3.0) < 5e-2
    assert abs(float((z.abs() > 1.959964).double().mean()) - 0.05) < 1e-3
    assert torch.equal(vf.add_noise(flux, err, 0.5, seed=1234), out)
    z2 = ((vf.add_noise(flux, err, 0.5, seed=1235) - flux) / (err * 0.5)).double()
    assert abs(float((z * z2).mean())) < 3e-3 and abs(float((z[:-1] * z[1:]).mean())) < 3e-3
    # a 2-D batch of the reference's shape, level 0 is the identity
    f2, e2 = flux[: 64 * 4096].view(64, 4096), err[: 64 * 4096].view(64, 4096)
    assert torch.equal(vf.add_noise(f2, e2, 0.0, seed=1), f2)


@pytest.mark.parametrize("core", [0, 1])
def test_gemm_colsum_out(dev, core):
    """colsum_out = column sums of the stored C (a bias gradient): fused in the ping-pong epilogue (core 1 = automatic on a
    256-aligned problem) or computed by the fallback pass (core 0); both must equal vit_colsum of the output."""
    import vit_amd.functional as vf
    from vit_amd import _cabi
    from vit_amd._cabi import ACT_DGELU

    M, N, K = 256 * 5, 768, 256
    dy, W, u = bf(randn((M, K), dev, 110)), bf(randn((K, N), dev, 111, 0.1)), bf(randn((M, N), dev, 112))
    _cabi.set_option("gemm_core", core)
    try:
        cs = torch.empty(N, device=dev)
        out = vf.gemm(dy, W, M=M, N=N, K=K, b_trans=True, act=ACT_DGELU, aux_in=u, colsum_out=cs)   # dX * gelu'(u)
        assert rel(cs, out.float().sum(0)) < 1e-5
        cs2 = torch.empty(N, device=dev)
        out2 = vf.gemm(dy, W, M=M, N=N, K=K, b_trans=True, colsum_out=cs2)                           # plain dX
        assert rel(cs2, out2.float().sum(0)) < 1e-5
        again = torch.empty(N, device=dev)
        vf.gemm(dy, W, M=M, N=N, K=K, b_trans=True, colsum_out=again)
        assert torch.equal(again, cs2)  # deterministic
    finally:
        _cabi.set_option("gemm_core", 1)


@pytest.mark.parametrize("core", [0, 1, 5])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_gemm_gelu_grad_and_mul_aux(dev, core, dt):
    """ACT_GELU_GRAD saves gelu'(pre-activation) in the forward, ACT_MUL_AUX multiplies by it in the backward: together they
    must reproduce autograd through F.gelu (every core; f32 operands run the split-bf16 kernel)."""
    import vit_amd.functional as vf
    from vit_amd import _cabi
    from vit_amd._cabi import ACT_GELU_GRAD, ACT_MUL_AUX

    M, N, K = 512, 768, 256
    cast = (lambda t: bf(t)) if dt == torch.bfloat16 else (lambda t: t)
    x, W, bias = cast(randn((M, K), dev, 120)), cast(randn((N, K), dev, 121, 0.1)), randn((N,), dev, 122)
    dy, W2 = cast(randn((M, K), dev, 123)), cast(randn((K, N), dev, 124, 0.1))
    _cabi.set_option("gemm_core", core)
    try:
        aux = torch.empty((M, N), dtype=dt, device=dev)
        y = vf.gemm(x, W, M=M, N=N, K=K, bias=bias, act=ACT_GELU_GRAD, aux_out=aux, out_dtype=dt)
        dU = vf.gemm(dy, W2, M=M, N=N, K=K, b_trans=True, act=ACT_MUL_AUX, aux_in=aux, out_dtype=dt)
    finally:
        _cabi.set_option("gemm_core", 1)
    pre = (x.float() @ W.float().t() + bias).requires_grad_(True)
    ref = F.gelu(pre)
    ref.backward(dy.float() @ W2.float())
    tol = 6e-3 if dt == torch.bfloat16 else 2e-5
    assert rel(y, ref.detach()) < tol
    assert rel(dU, pre.grad) < (8e-3 if dt == torch.bfloat16 else 3e-5)


@pytest.mark.parametrize("B,H,T,dh", [(3, 2, 129, 16), (4, 3, 197, 64), (2, 4, 50, 32), (2, 8, 122, 4)])
def test_attention_bwd_fused_colsum(dev, B, H, T, dh):
    """vit_attention_bwd with dqkv_colsum: the per-wave column sums the resident kernels emit, reduced over the batch, must equal
    vit_colsum over the stored dqkv (same bf16-rounded values, f32 sums), with and without dropout, for 1 and 2
    workgroups per head."""
    import vit_amd.functional as vf
    from vit_amd import _cabi

    D = H * dh
    qkv = bf(randn((B * T, 3 * D), dev, 140, 0.5))
    dctx = bf(randn((B * T, D), dev, 141, 0.5))
    for split in (1, 2):
        _cabi.set_option("attn_split", split)
        try:
            for drop in ((0.0, 0, 0), (0.1, 9, 3)):
                ctx, lse = vf.attention_fwd(qkv, B, H, T, dh, dh ** -0.5, dropout=drop)
                ref = vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, dh ** -0.5, dropout=drop)
                cs = torch.empty(3 * D, device=dev)
                out = vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, dh ** -0.5, dropout=drop, colsum_out=cs)
                assert torch.equal(out, ref)
                assert rel(cs, vf.colsum(ref)) < 1e-5
        finally:
            _cabi.set_option("attn_split", 2)


@pytest.mark.parametrize("M,N,K", [(256 * 100, 768, 256), (256 * 197, 768, 768), (256 * 90, 1024, 512),
                                   (256 * 73, 1024, 4096), (256 * 73, 1024, 3072), (256 * 70, 1024, 4096)])
def test_gemm_partial_last_round(dev, M, N, K):
    """Tile counts that leave a partial last round on 256 workgroups, short-K (300, 591, 360 tiles) and long-K (ViT-L: 292 =
    one round + 36; 280 = 256 + 24): those tiles run in the same single launch as the full rounds.  The forward (bias +
    dropout, bias, plain, GELU with its saved derivative) and the dX layout against the fp32 references, on the whole output
    and on the rows of the last tiles; the dropout zeros where the mask drops; two runs equal bit for bit."""
    import vit_amd.functional as vf
    from vit_amd._cabi import ACT_GELU_GRAD

    scale = 0.1 if K <= 1024 else 0.05
    x, W = bf(randn((M, K), dev, 150)), bf(randn((N, K), dev, 151, scale))
    bias = randn((N,), dev, 152)
    dy, W2 = bf(randn((M, K), dev, 153)), bf(randn((K, N), dev, 154, scale))
    drop = (0.1, 5, 6)

    def run():
        aux = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        return (vf.gemm(x, W, M=M, N=N, K=K, bias=bias, dropout=drop),
                vf.gemm(x, W, M=M, N=N, K=K, bias=bias),
                vf.gemm(x, W, M=M, N=N, K=K),
                vf.gemm(dy, W2, M=M, N=N, K=K, b_trans=True),
                vf.gemm(x, W, M=M, N=N, K=K, bias=bias, act=ACT_GELU_GRAD, aux_out=aux), aux)

    outs = run()
    for a, b in zip(outs, run()):
        assert torch.equal(a, b)
    yd, yb, y, dx, yg, aux = outs
    prod = x.float() @ W.float().t()
    pre = (prod + bias).requires_grad_(True)
    gelu = F.gelu(pre)
    gelu.sum().backward()  # pre.grad = gelu'(pre)
    mask = vf.dropout_bwd_cast(torch.ones((M, N), device=dev), drop).float()
    assert torch.equal(yd == 0, mask == 0)  # same dropout mask
    assert rel(yd, pre.detach() * mask) < 5e-3  # mask scale is bf16-rounded in this reconstruction
    ref_dx = dy.float() @ W2.float()
    tail = slice(M - 256 * 12, M)  # rows of the last tiles: the partial last round
    for out, ref in ((yb, pre.detach()), (y, prod), (dx, ref_dx)):
        assert rel(out, ref) < 4e-3
        assert rel(out[tail], ref[tail]) < 4e-3
    assert rel(yg, gelu.detach()) < 6e-3
    assert rel(aux, pre.grad) < 4e-3


@pytest.mark.parametrize("B,H,T,dh", [(1, 2, 197, 64), (1, 2, 577, 64), (1, 1, 640, 64)])
def test_attention_delta_residual(dev, B, H, T, dh):
    """vit_attention_fwd / vit_attention_bwd with ctx_lo: with value rows that share a large common component (what deep layers
    of a transformer look like), delta = rowsum(dO * O) from the 8-bit O is off by an amount common to each score row, which
    the sum over keys in dQ / dK does not average out.  The stored residual O - bf16(O) must (a) reconstruct O to 2^-15,
    (b) leave ctx itself unchanged, (c) bring dQ / dK to the level of the fp32 formula -- resident (197, 577) and tiled
    (640) kernels."""
    import vit_amd.functional as vf

    scale = dh ** -0.5
    qkv = randn((B * T, 3, H, dh), dev, 60, 0.5)
    qkv[:, 2] += 8.0 * randn((1, H, dh), dev, 61)  # common component of every value row
    qkv = bf(qkv.reshape(B * T, 3 * H * dh))
    ctx0, lse0 = vf.attention_fwd(qkv, B, H, T, dh, scale)
    lo = torch.empty_like(ctx0)
    ctx, lse = vf.attention_fwd(qkv, B, H, T, dh, scale, ctx_lo=lo)
    assert torch.equal(ctx, ctx0) and torch.equal(lse, lse0)
    q32 = qkv.double().requires_grad_(True)
    ref, _, _ = attn_ref(q32, B, H, T, dh, scale)
    # bf16 probabilities feed the PV product, so O itself carries ~2e-3; the residual must capture the ROUNDING of that O
    assert rel(ctx.double() + lo.double(), ref) < rel(ctx, ref)
    assert float((lo.float().abs() <= ctx.float().abs() * 2.0 ** -8 + 1e-30).float().mean()) == 1.0
    dctx = bf(randn((B * T, H * dh), dev, 62))
    ref.backward(dctx.double())
    g = q32.grad.view(B * T, 3, H * dh)
    d0 = vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, scale).double().view(B * T, 3, H * dh)
    d1 = vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, scale, ctx_lo=lo).double().view(B * T, 3, H * dh)
    e0 = [rel(d0[:, i], g[:, i]) for i in range(3)]
    e1 = [rel(d1[:, i], g[:, i]) for i in range(3)]
    print(f"[T={T}] dq/dk/dv rel err without residual {e0[0]:.2e}/{e0[1]:.2e}/{e0[2]:.2e}, with {e1[0]:.2e}/{e1[1]:.2e}/{e1[2]:.2e}")
    assert e1[0] < 0.5 * e0[0] and e1[1] < 0.5 * e0[1], (e0, e1)
    assert max(e1) < 1.5e-2, e1


@pytest.mark.parametrize("B,H,T,dh", [(2, 2, 129, 16), (2, 3, 197, 64), (1, 2, 224, 64), (1, 2, 240, 32), (3, 1, 17, 64), (1, 2, 64, 64),
                                      (40, 12, 197, 64), (300, 1, 130, 64), (2, 3, 208, 64), (3, 2, 65, 64), (2, 2, 96, 64),
                                      (64, 5, 177, 64),  # (40, 12, ..), (300, 1, ..), (64, 5, ..): several heads per persistent workgroup
                                      # more heads than CUs at padded lengths R = 64, 96, 128, 160, 80, 112: the pair-pipelined kernel issues
                                      # K / V pieces of the NEXT head in a head's LAST iteration there (none at R = 144, 176, 192, 208)
                                      # and must wait for them before its closing barrier (r03 advisor finding: read-before-wait)
                                      (300, 1, 64, 64), (300, 1, 96, 64), (300, 1, 128, 64), (300, 1, 160, 64), (150, 2, 75, 64),
                                      (300, 1, 100, 64)])
@pytest.mark.parametrize("drop", [(0.0, 0, 0), (0.1, 7, 5)])
def test_attention_bwd_fused_matches_two_kernel_path(dev, B, H, T, dh, drop):
    """The single-kernel backward (one workgroup per head; dS through the LDS) against the dQ + dK/dV pair: same dropout
    masks, same delta, so the results agree to bf16 rounding of differently ordered sums; column sums likewise; and both
    against fp64 autograd."""
    import vit_amd.functional as vf
    from vit_amd import _cabi

    scale = dh ** -0.5
    qkv = bf(randn((B * T, 3 * H * dh), dev, 70))
    lo = torch.empty((B * T, H * dh), dtype=torch.bfloat16, device=dev)
    ctx, lse = vf.attention_fwd(qkv, B, H, T, dh, scale, dropout=drop, ctx_lo=lo)
    dctx = bf(randn((B * T, H * dh), dev, 71))
    out = {}
    try:
        # two-kernel path and the pair-pipelined single kernel (dh 64, 64 <= T <= 208; elsewhere 4 is the two-kernel path too)
        for fused in (0, 4):
            _cabi.set_option("attn_bwd_fused", fused)
            cs = torch.zeros(3 * H * dh, device=dev)
            delta = torch.zeros((B * H, T), device=dev)
            d = vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, scale, dropout=drop, colsum_out=cs, ctx_lo=lo, delta=delta)
            out[fused] = (d.clone(), cs.clone(), delta.clone())
    finally:
        _cabi.set_option("attn_bwd_fused", 4)
    a, b_ = out[0], out[4]
    assert rel(b_[0], a[0]) < 6e-3, rel(b_[0], a[0])
    assert rel(b_[2], a[2]) < 1e-5
    assert rel(b_[1], b_[0].float().sum(0)) < 1e-5  # column sums of what was stored
    if drop[0] == 0.0:
        q64 = qkv.double().requires_grad_(True)
        ref, _, _ = attn_ref(q64, B, H, T, dh, scale)
        ref.backward(dctx.double())
        g = q64.grad.view(B * T, 3, H * dh)
        dd = b_[0].double().view(B * T, 3, H * dh)
        for i in range(3):
            assert rel(dd[:, i], g[:, i]) < 1.2e-2, (i, rel(dd[:, i], g[:, i]))


@pytest.mark.parametrize("H,dh", [(4, 64), (8, 32), (16, 16), (2, 128)])
@pytest.mark.parametrize("M,T", [(512, 197), (1024, 128)])
def test_gemm_rope_epilogue(dev, H, dh, M, T):
    """r04 ('RoPE on Q / K fused into K3's epilogue'; src/models/vit_with_rope.py:58-60, rope.py:116-131): vit_gemm
    with the rope fields rotates the q / k columns of a fused QKV projection.  On the ping-pong core (tile-aligned problem, head_dim
    16 / 32 / 64) that happens INSIDE the epilogue, on the f32 sums before the one rounding to bf16 -- the kernel symbol says so --
    and for every other case (head_dim 128 here; unaligned shapes; f32 operands) the library runs vit_rope_qk behind the product.
    Both against an fp64 projection + rotate_half rotation; the fused form must be at least as close as product-then-pass."""
    import vit_amd.functional as vf
    from vit_amd import _cabi

    D = H * dh
    K = 256
    x = bf(randn((M, K), dev, 300, 0.5))
    W = bf(randn((3 * D, K), dev, 301, 0.1))
    bias = randn((3 * D,), dev, 302)
    inv = 1.0 / (10000.0 ** (torch.arange(0, dh, 2).float() / dh))
    fr = torch.outer(torch.arange(T).float(), inv)
    cos, sin = fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)
    out = vf.gemm(x, W, M=M, N=3 * D, K=K, bias=bias, rope=(cos, sin, T, dh, 2 * D))
    sym = _cabi.load().vit_last_gemm_kernel().decode()
    assert ("<0, 0, 8, 8>" in sym) == (dh <= 64), sym  # the rotating epilogue wherever a wave's 64 columns are whole heads
    # fp64 reference
    y = x.double() @ W.double().t() + bias.double()
    t = (torch.arange(M, device=dev) % T)
    c, s = cos.double()[t], sin.double()[t]                      # [M, dh/2]
    ref = y.clone()
    for part in range(2):
        blk = y[:, part * D:(part + 1) * D].view(M, H, dh)
        x1, x2 = blk[..., : dh // 2], blk[..., dh // 2:]
        rot = torch.cat([x1 * c[:, None] - x2 * s[:, None], x2 * c[:, None] + x1 * s[:, None]], -1)
        ref[:, part * D:(part + 1) * D] = rot.reshape(M, D)
    e_fused = rel(out, ref)
    assert e_fused < 4e-3, e_fused
    assert rel(out[:, 2 * D:], y[:, 2 * D:]) < 4e-3  # the v third is the plain projection
    # product, then the separate pass (what every round before did): rounds twice
    two = vf.gemm(x, W, M=M, N=3 * D, K=K, bias=bias)
    vf.rope_qk(two, cos, sin, T, H, dh)
    e_two = rel(two, ref)
    assert e_fused <= e_two * 1.02 + 1e-6, (e_fused, e_two)
    if dh > 64:
        assert torch.equal(out, two)  # the library's own fall-back IS that pass
