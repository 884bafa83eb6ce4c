"""Every dropout mask a HIP kernel draws, against the host restatement oracle/dropmask.py -- not against another kernel.

The masks are a pure function of (seed, site, row, column) (vit_amd/csrc/common.h:56-112) and the backward regenerates
each one in a different kernel from the one that applied it in the forward, so each kernel is checked on its own:
  * GEMM epilogues and the elementwise kernels bit for bit (integer-valued operands make every accumulation exact);
  * attention forward: the multiplier recovered with Q = K = 0 (uniform probabilities) and a one-hot V, thresholded at
    half the scale, equals keep_mask bit for bit, on every forward form of the dispatch (attn_plan in attention.hip);
  * attention backward: with Q = K = V = 0 and a one-hot dO block, dV[k, d] = M[i*dh + d, k] / T recovers the backward's
    own mask, on every backward form of attention_bwd_impl; the dS path against fp64 autograd with the restated mask;
  * the bound per-step record (vit_step_state_bind / vit_step_advance) of the captured step."""
import math

import numpy as np
import pytest
import torch

from oracle import dropmask as dm

pytestmark = pytest.mark.gpu

P = 0.1


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def mult(p, seed, site, rows, cols, dev, keys_xor=None):
    return torch.from_numpy(dm.multiplier(dm.drop_cfg(p, seed, site), rows, cols, keys_xor=keys_xor)).to(dev)


def keep(p, seed, site, rows, cols, keys_xor=None):
    return torch.from_numpy(dm.keep_mask(dm.drop_cfg(p, seed, site), rows, cols, keys_xor=keys_xor))


def ints(shape, dev, seed, lo=-2, hi=2, dtype=torch.bfloat16):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device=dev).to(dtype)


def eighths(n, dev, seed):
    """Odd multiples of 1/8 in [-15/8, 15/8]: never an integer, so acc + bias is never 0 and every dropped element shows."""
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randint(-8, 8, (n,), generator=g, device=dev) * 2 + 1).float() / 8


def randn(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


class option:
    """A process-wide vit_set_option knob for the duration of a block (put back to its default afterwards)."""

    DEFAULTS = {"gemm_core": 1, "attn_split": 2, "attn_bwd_fused": 4}

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from vit_amd import _cabi

        _cabi.set_option(self.name, self.value)

    def __exit__(self, *exc):
        from vit_amd import _cabi

        _cabi.set_option(self.name, self.DEFAULTS[self.name])
        return False


def equal_either(out, e_plain, e_fma):
    """Bitwise equality with the plainly rounded expectation or, where a residual is added behind the dropout multiply,
    with its fused multiply-add form (the compiler may contract v * k + r)."""
    return bool(((out == e_plain) | (out == e_fma)).all())


# ------------------------------------------------------------------ GEMM epilogues, bit exact
def _gemm_case(dev, M, N, K, *, seed, site, out_dtype=torch.bfloat16, opdt=torch.bfloat16, residual=False,
               row_map=None, handle=None, keys_xor=None):
    import vit_amd.functional as vf

    A, W = ints((M, K), dev, 1000 + M % 997, dtype=opdt), ints((N, K), dev, 2000 + K, dtype=opdt)
    bias = eighths(N, dev, 3)
    acc = (A.double() @ W.double().t()).float()  # integers below 2^15: exact in any order
    v = acc + bias                               # exact: 19 significant bits
    if row_map is None:
        rows, out_row = M, torch.arange(M, device=dev)
    else:
        rpb, orb, roff = row_map
        rows = (M // rpb) * orb
        m = torch.arange(M, device=dev)
        out_row = (m // rpb) * orb + m % rpb + roff
    res = randn((rows, N), dev, 5).float() if residual else None
    out = torch.full((rows, N), 7.0, dtype=out_dtype, device=dev)
    kw = dict(M=M, N=N, K=K, out=out, bias=bias, dropout=(P, seed, site), residual=res)
    if row_map is not None:
        kw["row_map"] = row_map
    if handle is not None:
        with vf.use_handle(handle):
            vf.gemm(A, W, **kw)
    else:
        vf.gemm(A, W, **kw)
    mk = mult(P, seed, site, rows, N, dev, keys_xor)[out_row]
    e_plain = v * mk
    e_fma = e_plain
    if residual:
        e_fma = (v.double() * mk.double() + res[out_row].double()).float()
        e_plain = e_plain + res[out_row]
    got = out[out_row]
    assert equal_either(got, e_plain.to(out_dtype), e_fma.to(out_dtype)), (M, N, K)
    if not residual:
        assert torch.equal(got == 0, mk == 0)
    if row_map is not None:  # rows the map does not reach are untouched
        untouched = torch.ones(rows, dtype=torch.bool, device=dev)
        untouched[out_row] = False
        assert bool((out[untouched] == 7.0).all())
    return out


@pytest.mark.parametrize("M,N,K,out_dtype,residual", [(1024, 768, 768, torch.bfloat16, False), (330, 256, 192, torch.float32, True),
                                                      (516, 96, 32, torch.bfloat16, False)])
def test_gemm_generic_core_dropout_exact(dev, M, N, K, out_dtype, residual):
    from vit_amd import _cabi

    with option("gemm_core", 0):
        _gemm_case(dev, M, N, K, seed=2 ** 63 + 11, site=6, out_dtype=out_dtype, residual=residual)
    assert _cabi.load().vit_last_gemm_kernel().decode().startswith("gemm_bf16_kernel")


@pytest.mark.parametrize("M,K", [(1024, 768), (1024, 3072), (256 * 197, 768), (256 * 197, 3072)])
def test_gemm_pingpong_dropout_epilogue_exact(dev, M, K):
    """The ViT-B out-projection / FC2 shapes on the ping-pong core: M a multiple of 256 (C3's padded B = 4, and B = 256),
    N = 768, bf16 out with bias + dropout -- the FAST == 3 epilogue (gemm2.hip:322)."""
    from vit_amd import _cabi

    _gemm_case(dev, M, 768, K, seed=12345, site=3 if K == 768 else 4)
    name = _cabi.load().vit_last_gemm_kernel().decode()
    assert name == "gemm3_kernel<0, 0, 3, 8>", name  # the ping-pong core's bias + dropout -> bf16 epilogue


@pytest.mark.parametrize("M,N,K", [(256 * 100, 768, 256), (256 * 73, 1024, 3072), (256 * 70, 1024, 4096)])
def test_gemm_partial_last_round_dropout_exact(dev, M, N, K):
    _gemm_case(dev, M, N, K, seed=5, site=6)


@pytest.mark.parametrize("M,N,K,out_dtype,residual", [(330, 256, 192, torch.float32, True), (1024, 768, 768, torch.float32, False),
                                                      (1024, 768, 768, torch.bfloat16, False)])
def test_gemm_x3_dropout_exact(dev, M, N, K, out_dtype, residual):
    """f32 operands: the split-bf16 x3 kernel (precision '32')."""
    _gemm_case(dev, M, N, K, seed=77, site=2, opdt=torch.float32, out_dtype=out_dtype, residual=residual)


@pytest.mark.parametrize("opdt", [torch.bfloat16, torch.float32])
def test_gemm_row_map_dropout_keyed_by_out_row(dev, opdt):
    """rows b*rpb + n are written to b*orb + n + roff; the mask is a function of the OUTPUT row (vit_amd.h)."""
    _gemm_case(dev, 6 * 55, 256, 192, seed=31, site=9, opdt=opdt, out_dtype=torch.float32, row_map=(55, 56, 1))


@pytest.mark.parametrize("reserve", [0, 8, 16, 40])
def test_gemm_reserve_cus_keeps_the_mask(dev, reserve):
    """The persistent tile walk changes with the CUs left to a collective; the mask must not."""
    from vit_amd import _cabi

    h = _cabi.Handle(dev.index or 0)
    h.set_option("reserve_cus", reserve)
    _gemm_case(dev, 256 * 100, 768, 256, seed=8, site=10, handle=h)
    _gemm_case(dev, 256 * 197, 768, 768, seed=8, site=11, handle=h)


# ------------------------------------------------------------------ elementwise kernels, bit exact
@pytest.mark.parametrize("rows,cols", [(256 * 197, 768), (1000, 32), (77, 1028)])
def test_dropout_bwd_cast_exact(dev, rows, cols):
    import vit_amd.functional as vf

    dx = randn((rows, cols), dev, 200)
    m = mult(P, 99, 7, rows, cols, dev)
    for odt in (torch.bfloat16, torch.float32):
        out = vf.dropout_bwd_cast(dx, (P, 99, 7), out_dtype=odt)
        assert torch.equal(out, (dx * m).to(odt)), odt


@pytest.mark.parametrize("B,T,D", [(256, 197, 768), (3, 129, 32), (5, 17, 64)])
@pytest.mark.parametrize("with_pos", [False, True])
def test_embed_finish_exact(dev, B, T, D, with_pos):
    import vit_amd.functional as vf

    tok = randn((B, T, D), dev, 210)
    cls, pos = randn((D,), dev, 211), (randn((T, D), dev, 212) if with_pos else None)
    seed = 2 ** 64 - 3
    out = vf.embed_finish(tok.clone(), cls, pos, dropout=(P, seed, 0))
    v = tok.clone()
    v[:, 0] = cls
    if pos is not None:
        v = v + pos
    m = mult(P, seed, 0, B * T, D, dev).view(B, T, D)
    assert torch.equal(out, v * m)


@pytest.mark.parametrize("B,T,D", [(256, 197, 768), (3, 129, 32), (20, 17, 64)])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_embed_finish_bwd_exact(dev, B, T, D, accumulate):
    import vit_amd.functional as vf

    h = vf._h(torch.empty(1, device=dev))
    h.ensure_workspace(min(B, 16) * T * D * 4)
    dtok = randn((B, T, D), dev, 220)
    m = mult(P, 41, 0, B * T, D, dev).view(B, T, D)
    g = dtok * m
    init_cls, init_pos = randn((D,), dev, 221), randn((T, D), dev, 222)
    for odt in (torch.bfloat16, torch.float32):
        dcls, dpos = init_cls.clone(), init_pos.clone()
        dpatch = torch.empty((B * (T - 1), D), dtype=odt, device=dev)
        from vit_amd._cabi import check
        from vit_amd.functional import _DT, _stream

        check(h.lib.vit_embed_finish_bwd(h.h, dtok.data_ptr(), dpatch.data_ptr(), _DT[odt], dcls.data_ptr(), dpos.data_ptr(),
                                         B, T, D, P, 41, 0, accumulate, _stream(dtok)), "vit_embed_finish_bwd")
        assert torch.equal(dpatch, g[:, 1:].reshape(B * (T - 1), D).to(odt))
        ref_cls = g[:, 0].double().sum(0) + (init_cls.double() if accumulate else 0)
        ref_pos = g.double().sum(0) + (init_pos.double() if accumulate else 0)
        assert rel(dcls, ref_cls) <= 1e-6 and rel(dpos, ref_pos) <= 1e-6, (rel(dcls, ref_cls), rel(dpos, ref_pos))


@pytest.mark.parametrize("rows,D", [(256 * 197, 768), (516, 32), (77, 1024)])
def test_layernorm_bwd_fused_dyn_exact(dev, rows, D):
    import vit_amd.functional as vf

    x = randn((rows, D), dev, 230) * 2 + 0.3
    g, b = randn((D,), dev, 231) * 0.1 + 1, randn((D,), dev, 232) * 0.1
    _, mean, rstd = vf.layernorm_fwd(x, g, b, 1e-12, out_dtype=torch.float32)
    dy, dres = vf.cast_f32_bf16(randn((rows, D), dev, 233)), randn((rows, D), dev, 234)
    E = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)
    seed, site = 2 ** 40 + 1, 10
    dx, _, _, dyn, dbias = vf.layernorm_bwd_fused(dy, x, g, mean, rstd, dres, E(rows, D), E(D), E(D),
                                                  E(rows, D, dt=torch.bfloat16), E(D), (P, seed, site))
    m = mult(P, seed, site, rows, D, dev)
    assert torch.equal(dyn, (m * dx).to(torch.bfloat16))
    assert rel(dbias, dyn.double().sum(0)) <= 1e-5


# ------------------------------------------------------------------ attention: recovered masks
def attn_keep_ref(drop, B, H, T, keys_xor=None):
    p, seed, site = drop
    return keep(p, seed, site, B * H * T, T, keys_xor).view(B, H, T, T)


def recover_fwd_mask(dev, B, H, T, dh, drop, dtype=torch.bfloat16):
    """Forward multiplier M[b,h,q,k]: Q = K = 0 gives probabilities 1/T; a one-hot V block makes ctx[q, d] = M[q, i*dh+d] / T."""
    import vit_amd.functional as vf

    mask = torch.zeros((B, H, T, T), device=dev)
    for i in range(math.ceil(T / dh)):
        n = min(dh, T - i * dh)
        qkv = torch.zeros((B, T, 3, H, dh), device=dev)
        d = torch.arange(n, device=dev)
        qkv[:, i * dh + d, 2, :, d] = 1.0
        ctx, _ = vf.attention_fwd(qkv.view(B * T, 3 * H * dh).to(dtype), B, H, T, dh, 1.0, dropout=drop)
        c = ctx.float().view(B, T, H, dh).permute(0, 2, 1, 3) * T
        mask[:, :, :, i * dh:i * dh + n] = c[..., :n]
    return mask


def recover_bwd_mask(dev, B, H, T, dh, drop, dtype=torch.bfloat16, ctx_lo=False, colsum=False):
    """Backward multiplier on the dV path: Q = K = V = 0 gives P = 1/T; dO[i*dh + d, d] = 1 makes dV[k, d] = M[i*dh + d, k] / T."""
    import vit_amd.functional as vf

    D = H * dh
    qkv = torch.zeros((B * T, 3 * D), dtype=dtype, device=dev)
    lo = torch.zeros((B * T, D), dtype=dtype, device=dev) if ctx_lo else None
    ctx, lse = vf.attention_fwd(qkv, B, H, T, dh, 1.0, dropout=drop, ctx_lo=lo)
    mask = torch.zeros((B, H, T, T), device=dev)
    for i in range(math.ceil(T / dh)):
        n = min(dh, T - i * dh)
        dO = torch.zeros((B, T, H, dh), device=dev)
        d = torch.arange(n, device=dev)
        dO[:, i * dh + d, :, d] = 1.0
        cs = torch.zeros(3 * D, device=dev) if colsum else None
        dqkv = vf.attention_bwd(qkv, ctx, dO.view(B * T, D).to(dtype), lse, B, H, T, dh, 1.0, dropout=drop, ctx_lo=lo,
                                colsum_out=cs)
        dv = dqkv.float().view(B, T, 3, H, dh)[:, :, 2].permute(0, 2, 3, 1)  # [B, H, dh (query i*dh + d), T (key)]
        mask[:, :, i * dh:i * dh + n, :] = dv[:, :, :n, :] * T
        if colsum:  # the fused column sums of the same call: dV column d sums M[i*dh + d, :] / T over keys and batches
            assert rel(cs, dqkv.float().sum(0)) < 1e-5
    return mask


def assert_keep_bits(mask, drop, B, H, T, keys_xor=None):
    scale = dm.thr_scale(drop[0])[1]
    got = (mask > 0.5 * scale).cpu()
    exp = attn_keep_ref(drop, B, H, T, keys_xor)
    bad = int((got != exp).sum())
    assert bad == 0, f"{bad} of {got.numel()} keep bits differ"
    # and the kept values carry the scale (to the output dtype's rounding)
    kept = mask[exp.to(mask.device)]
    assert float((kept - scale).abs().max()) < 2e-2 * scale


# (B, H, T, dh, dtype, what) -- every forward form of vit_attention_fwd
FWD_FORMS = [
    (2, 12, 197, 64, torch.bfloat16, "resident <64,RQ,true,208,12,2,4> (attn_split 2) / <64,RQ,true> (split 1)"),
    (24, 12, 197, 64, torch.bfloat16, "ViT-B heads, B*H = 288 > 256"),
    (1, 16, 129, 64, torch.bfloat16, "resident dh 64"),
    (1, 16, 577, 64, torch.bfloat16, "resident dh 64 at the ViT-L length"),
    (2, 4, 122, 4, torch.bfloat16, "dh 4: tiled (8-byte head offsets)"),
    (2, 4, 129, 8, torch.bfloat16, "resident dh <= 32"),
    (2, 2, 129, 16, torch.bfloat16, "resident dh <= 32"),
    (1, 2, 150, 48, torch.bfloat16, "resident 32 < dh < 64"),
    (1, 2, 700, 12, torch.bfloat16, "tiled"),
    (1, 1, 70, 128, torch.bfloat16, "tiled dh 128"),
    (1, 2, 197, 64, torch.float32, "f32 attn32m"),
    (2, 2, 129, 16, torch.float32, "f32 attn32_row"),
]


def _resident(f):
    B, H, T, dh, dtype, _ = f
    return dtype == torch.bfloat16 and dh in (8, 16, 48, 64) and T <= 592


# attn_split (workgroups per head) only changes the resident bf16 kernels: both values there, the default elsewhere
@pytest.mark.parametrize("B,H,T,dh,dtype,what,split", [f + (s,) for f in FWD_FORMS for s in ((1, 2) if _resident(f) else (2,))])
def test_attention_fwd_keep_bits(dev, B, H, T, dh, dtype, what, split):
    drop = (P, 2 ** 63 + 99, 5)
    with option("attn_split", split):
        mask = recover_fwd_mask(dev, B, H, T, dh, drop, dtype)
    assert_keep_bits(mask, drop, B, H, T)


# (B, H, T, dh, dtype, ctx_lo, attn_bwd_fused, colsum, reserve_cus, what) -- every backward form of attention_bwd_impl
BWD_FORMS = [
    (2, 12, 197, 64, torch.bfloat16, True, 4, False, -1, "pipe <true,12,true>"),
    (2, 12, 197, 64, torch.bfloat16, False, 4, False, -1, "pipe <true,0,false>"),
    (2, 3, 129, 64, torch.bfloat16, False, 4, False, -1, "pipe <false,0,false>"),
    (2, 3, 197, 64, torch.bfloat16, False, 0, False, -1, "resident dQ + dK/dV pair"),
    (1, 16, 577, 64, torch.bfloat16, True, 4, False, -1, "resident pair at T 577"),
    (2, 2, 129, 16, torch.bfloat16, False, 4, False, -1, "resident pair dh 16"),
    (1, 2, 700, 12, torch.bfloat16, False, 4, False, -1, "tiled pair"),
    (1, 1, 70, 128, torch.bfloat16, False, 4, False, -1, "tiled pair dh 128"),
    (1, 2, 197, 64, torch.float32, False, 4, False, -1, "f32 attn32m"),
    (2, 2, 129, 16, torch.float32, False, 4, False, -1, "f32 attn32_row"),
    (2, 12, 197, 64, torch.bfloat16, True, 4, True, -1, "colsum entry point, pipe"),
    (2, 3, 197, 64, torch.bfloat16, False, 0, True, -1, "colsum entry point, resident pair"),
    (24, 12, 197, 64, torch.bfloat16, True, 4, False, 16, "pipe, B*H = 288 > 256, reserve_cus 16"),
    (24, 12, 197, 64, torch.bfloat16, False, 0, False, 16, "resident pair, B*H = 288, reserve_cus 16"),
]


def _with_handle(dev, reserve):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    if reserve < 0:
        return None, None
    h = _cabi.Handle(dev.index or 0)
    h.set_option("reserve_cus", reserve)
    return h, vf.use_handle(h)


@pytest.mark.parametrize("B,H,T,dh,dtype,ctx_lo,fused,colsum,reserve,what", BWD_FORMS)
def test_attention_bwd_keep_bits(dev, B, H, T, dh, dtype, ctx_lo, fused, colsum, reserve, what):
    drop = (P, 424242, 9)
    h, ctxm = _with_handle(dev, reserve)
    with option("attn_bwd_fused", fused):
        if ctxm is not None:
            with ctxm:
                mask = recover_bwd_mask(dev, B, H, T, dh, drop, dtype, ctx_lo=ctx_lo, colsum=colsum)
        else:
            mask = recover_bwd_mask(dev, B, H, T, dh, drop, dtype, ctx_lo=ctx_lo, colsum=colsum)
    assert_keep_bits(mask, drop, B, H, T)


def attn_ref64(qkv, B, H, T, dh, scale, m):
    q, k, v = qkv.view(B, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    p = ((q @ k.transpose(-1, -2)) * scale).softmax(-1)
    return ((p * m) @ v).permute(0, 2, 1, 3).reshape(B * T, H * dh)


DS_FORMS = [f[:10] for f in BWD_FORMS if f[8] < 0 and not f[7]] + [(24, 12, 197, 64, torch.bfloat16, True, 4, False, 16, "")]


@pytest.mark.parametrize("B,H,T,dh,dtype,ctx_lo,fused,colsum,reserve,what", DS_FORMS)
def test_attention_bwd_ds_path_matches_restated_mask(dev, B, H, T, dh, dtype, ctx_lo, fused, colsum, reserve, what):
    """dQ / dK (the dS path) and dV on random inputs against fp64 autograd with the restated multiplier, at the 1.5e-2 gate
    of the attention tests (f32: 2e-5); the same against the mask of site + 1 must be at least 10x worse."""
    import vit_amd.functional as vf

    drop = (P, 777, 13)
    scale = dh ** -0.5
    qkv = randn((B * T, 3 * H * dh), dev, 240, 0.7).to(dtype)
    dctx = randn((B * T, H * dh), dev, 241).to(dtype)
    lo = torch.empty((B * T, H * dh), dtype=dtype, device=dev) if ctx_lo else None
    h, ctxm = _with_handle(dev, reserve)
    with option("attn_bwd_fused", fused):
        if ctxm is not None:
            ctxm.__enter__()
        try:
            ctx, lse = vf.attention_fwd(qkv, B, H, T, dh, scale, dropout=drop, ctx_lo=lo)
            dqkv = vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, scale, dropout=drop, ctx_lo=lo)
        finally:
            if ctxm is not None:
                ctxm.__exit__(None, None, None)
    got = dqkv.double().view(B * T, 3, H * dh)
    tol = 2e-5 if dtype == torch.float32 else 1.5e-2
    errs = {}
    for s in (drop[2], drop[2] + 1):
        m = torch.from_numpy(dm.attn_multiplier(dm.drop_cfg(P, drop[1], s), B, H, T)).to(dev).double()
        x = qkv.double().requires_grad_(True)
        ref = attn_ref64(x, B, H, T, dh, scale, m)
        ref.backward(dctx.double())
        g = x.grad.view(B * T, 3, H * dh)
        errs[s] = [rel(got[:, i], g[:, i]) for i in range(3)]
        if s == drop[2]:
            assert rel(ctx, ref.detach()) < (1e-5 if dtype == torch.float32 else 6e-3)
    right, wrong = errs[drop[2]], errs[drop[2] + 1]
    print(f"[{what}] dq/dk/dv rel err {right}, against the mask of site + 1: {wrong}")
    assert max(right) < tol, right
    for i in range(3):
        assert wrong[i] >= 10 * right[i], (i, right, wrong)


# ------------------------------------------------------------------ the bound per-step record
def _record_view(state):
    u = state.cpu().numpy().view(np.uint32)
    f = state.cpu().numpy().view(np.float32)
    return int(u[0]), int(u[1]), f[3], f[4], int(u[5])


def test_step_advance_record(dev):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    h = _cabi.Handle(dev.index or 0)
    base = 0x7EDCBA9876543210
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    state[5] = 4
    _cabi.check(h.lib.vit_step_state_bind(h.h, state.data_ptr()), "vit_step_state_bind")
    try:
        _cabi.check(h.lib.vit_step_advance(h.h, base, 0.9, 0.999, vf._stream(state)), "vit_step_advance")
        torch.cuda.synchronize(dev)
    finally:
        _cabi.check(h.lib.vit_step_state_bind(h.h, None), "vit_step_state_bind")
    k0, k1, bc1, rbc2, step = _record_view(state)
    e0, e1, ebc1, erbc2, estep = dm.step_record(base, 5)
    assert (k0, k1, step) == (e0, e1, estep)
    assert bc1.tobytes() == np.float32(ebc1).tobytes() and rbc2.tobytes() == np.float32(erbc2).tobytes(), (bc1, ebc1, rbc2, erbc2)


def test_bound_record_keys_reach_every_kernel_kind(dev):
    """While a record is bound, a GEMM, an elementwise kernel, the LayerNorm backward, the attention forward and the attention
    backward all draw keep_mask(..., keys_xor = the record's keys); with p = 0 the record changes nothing."""
    import vit_amd.functional as vf
    from vit_amd import _cabi

    h = _cabi.Handle(dev.index or 0)
    base, step = 0x1234567, 7
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    state[5] = step - 1
    kx = dm.step_keys(base, step)
    seed = 55
    _cabi.check(h.lib.vit_step_state_bind(h.h, state.data_ptr()), "vit_step_state_bind")
    try:
        with vf.use_handle(h):
            _cabi.check(h.lib.vit_step_advance(h.h, base, 0.9, 0.999, vf._stream(state)), "vit_step_advance")
            # GEMM (ping-pong epilogue) and generic core
            _gemm_case(dev, 1024, 768, 768, seed=seed, site=3, handle=h, keys_xor=kx)
            with option("gemm_core", 0):
                _gemm_case(dev, 330, 256, 192, seed=seed, site=3, handle=h, keys_xor=kx, out_dtype=torch.float32)
            # elementwise
            dx = randn((512, 768), dev, 250)
            out = vf.dropout_bwd_cast(dx, (P, seed, 4), out_dtype=torch.float32)
            assert torch.equal(out, dx * mult(P, seed, 4, 512, 768, dev, kx))
            assert not torch.equal(out, dx * mult(P, seed, 4, 512, 768, dev))
            # LayerNorm backward
            rows, D = 300, 256
            x = randn((rows, D), dev, 251)
            g, b = randn((D,), dev, 252) * 0.1 + 1, randn((D,), dev, 253) * 0.1
            _, mean, rstd = vf.layernorm_fwd(x, g, b, 1e-12, out_dtype=torch.float32)
            E = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)
            dx1, _, _, dyn, _ = vf.layernorm_bwd_fused(vf.cast_f32_bf16(randn((rows, D), dev, 254)), x, g, mean, rstd, None,
                                                       E(rows, D), E(D), E(D), E(rows, D, dt=torch.bfloat16), E(D), (P, seed, 6))
            assert torch.equal(dyn, (mult(P, seed, 6, rows, D, dev, kx) * dx1).to(torch.bfloat16))
            # attention forward / backward (pipe kernel, ViT-B heads)
            drop = (P, seed, 1)
            assert_keep_bits(recover_fwd_mask(dev, 1, 12, 197, 64, drop), drop, 1, 12, 197, keys_xor=kx)
            assert_keep_bits(recover_bwd_mask(dev, 1, 12, 197, 64, drop, ctx_lo=True), drop, 1, 12, 197, keys_xor=kx)
            # p = 0: the record is not consulted
            dx0 = vf.dropout_bwd_cast(dx, (0.0, seed, 4), out_dtype=torch.float32)
            assert torch.equal(dx0, dx)
            qkv = randn((2 * 129, 3 * 64), dev, 255).to(torch.bfloat16)
            c_bound, _ = vf.attention_fwd(qkv, 2, 1, 129, 64, 0.125, dropout=(0.0, seed, 1))
        torch.cuda.synchronize(dev)
    finally:
        _cabi.check(h.lib.vit_step_state_bind(h.h, None), "vit_step_state_bind")
    c_free, _ = vf.attention_fwd(qkv, 2, 1, 129, 64, 0.125)
    assert torch.equal(c_bound, c_free)
