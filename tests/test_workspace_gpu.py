"""The workspace contract of include/vit_amd.h on the MI355X: a call that needs more workspace than its handle holds returns
VIT_ERR_WORKSPACE before it launches anything and says how much it needs; Handle.call grows the workspace and repeats the call;
and no result depends on how large the workspace was -- kernels and summation order follow from the shape and the options."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

WS = -4
SENTINEL = 7.0  # exact in bf16 and f32


def randn(shape, dev, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(dev).to(dtype)


def filled(shape, dev, dtype=torch.float32):
    return torch.full(shape, SENTINEL, dtype=dtype, device=dev)


def untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool((t == SENTINEL).all()) for t in tensors)


def handle(dev, workspace_bytes=None, **options):
    from vit_amd import _cabi

    idx = dev.index or 0
    h = _cabi.Handle(idx) if workspace_bytes is None else _cabi.Handle(idx, workspace_bytes=workspace_bytes)
    for name, value in options.items():
        h.set_option(name, value)
    return h


_attn = {}


def attn_inputs(dev, B, H, T, dh):
    """qkv, ctx, dctx, lse of one attention shape (forward through the default handle), computed once and only read."""
    import vit_amd.functional as vf

    key = (B, H, T, dh)
    if key not in _attn:
        qkv = randn((B * T, 3 * H * dh), dev, 300 + T + dh, torch.bfloat16)
        ctx, lse = vf.attention_fwd(qkv, B, H, T, dh, dh ** -0.5)
        _attn[key] = (qkv, ctx, randn((B * T, H * dh), dev, 301 + T + dh, torch.bfloat16), lse)
    return _attn[key]


# ---------------------------------------------------------------------------------- (a) nothing launched on a short workspace
def test_short_workspace_launches_nothing(dev):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    h = handle(dev, 0)
    lib, st = h.lib, vf._stream(torch.empty(1, device=dev))
    BF, F32 = _cabi.VIT_BF16, _cabi.VIT_F32

    def refused(rc, *outputs):
        assert rc == WS, (rc, lib.vit_last_error())
        assert untouched(*outputs)
        assert lib.vit_workspace_needed() > 0

    # vit_gemm, split-K weight gradient 256 x 256 x 4096
    dy, x = randn((4096, 256), dev, 1, torch.bfloat16), randn((4096, 256), dev, 2, torch.bfloat16)
    dW = filled((256, 256), dev)
    d = _cabi.GemmDesc()
    d.M, d.N, d.K, d.a_trans, d.b_trans, d.ab_dtype = 256, 256, 4096, 1, 1, BF
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.c_dtype = dy.data_ptr(), 256, x.data_ptr(), 256, dW.data_ptr(), 256, F32
    d.alpha, d.split_k = 1.0, -1
    refused(lib.vit_gemm(h.h, ctypes.byref(d), st), dW)

    # vit_gemm with colsum_out, 512 x 256 x 256 on the ping-pong core
    a, b = randn((512, 256), dev, 3, torch.bfloat16), randn((256, 256), dev, 4, torch.bfloat16)
    c, cs = filled((512, 256), dev, torch.bfloat16), filled((256,), dev)
    d = _cabi.GemmDesc()
    d.M, d.N, d.K, d.b_trans, d.ab_dtype = 512, 256, 256, 1, BF
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.c_dtype = a.data_ptr(), 256, b.data_ptr(), 256, c.data_ptr(), 256, BF
    d.alpha, d.colsum_out = 1.0, cs.data_ptr()
    refused(lib.vit_gemm(h.h, ctypes.byref(d), st), c, cs)

    # vit_attention_bwd with column sums (the pipelined form)
    B, H, T, dh = 2, 4, 65, 64
    qkv, ctx, dctx, lse = attn_inputs(dev, B, H, T, dh)
    delta, dqkv, cs = filled((B * H, T), dev), filled(tuple(qkv.shape), dev, torch.bfloat16), filled((3 * H * dh,), dev)
    refused(lib.vit_attention_bwd(h.h, qkv.data_ptr(), ctx.data_ptr(), None, dctx.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                  dqkv.data_ptr(), BF, B, H, T, dh, dh ** -0.5, 0.0, 0, 0, cs.data_ptr(), st), delta, dqkv, cs)

    # vit_layernorm_bwd_fused, 64 x 64
    xs, g = randn((64, 64), dev, 5), randn((64,), dev, 6)
    mean, rstd, dyl = randn((64,), dev, 7), randn((64,), dev, 8).abs() + 0.5, randn((64, 64), dev, 9, torch.bfloat16)
    dx, dg, db, dyn, dbias = (filled((64, 64), dev), filled((64,), dev), filled((64,), dev),
                              filled((64, 64), dev, torch.bfloat16), filled((64,), dev))
    refused(lib.vit_layernorm_bwd_fused(h.h, dyl.data_ptr(), BF, xs.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                        None, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), 64, 64, dyn.data_ptr(), BF,
                                        dbias.data_ptr(), 0.1, 5, 6, st), dx, dg, db, dyn, dbias)

    # vit_colsum_rows in the order of the ping-pong epilogue's sums
    rows_a, out = randn((4, 256), dev, 10, torch.bfloat16), filled((256,), dev)
    refused(lib.vit_colsum_rows(h.h, rows_a.data_ptr(), BF, 256, out.data_ptr(), 4, 256, 64, 256, st), out)

    # vit_cov_accumulate over two row slices (a shape of tests/test_covstats_gpu.py)
    xc, mu, acc = randn((300, 200), dev, 11), randn((200,), dev, 12), filled((200, 200), dev)
    refused(lib.vit_cov_accumulate(h.h, xc.data_ptr(), 200, mu.data_ptr(), acc.data_ptr(), 300, 200, st), acc)
    assert h.workspace_bytes == 0


# ---------------------------------------------------------------------------------- (b) same bits whatever the workspace was
def _gemm_dw(dev):
    import vit_amd.functional as vf

    dy, x = randn((4096, 256), dev, 21, torch.bfloat16), randn((4096, 256), dev, 22, torch.bfloat16)
    return lambda: [vf.linear_bwd_dw(dy, x)]


def _gemm_colsum(dev, M, N, K):
    import vit_amd.functional as vf

    a, b = randn((M, K), dev, 23, torch.bfloat16), randn((K, N), dev, 24, torch.bfloat16)

    def run():
        cs = torch.empty(N, device=dev)
        return [vf.gemm(a, b, M=M, N=N, K=K, b_trans=True, colsum_out=cs), cs]
    return run


def _attention_bwd(dev, B, H, T, dh):
    import vit_amd.functional as vf

    qkv, ctx, dctx, lse = attn_inputs(dev, B, H, T, dh)

    def run():
        cs, delta = torch.empty(3 * H * dh, device=dev), torch.empty((B * H, T), device=dev)
        return [vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, dh ** -0.5, delta=delta, colsum_out=cs), cs, delta]
    return run


def _layernorm_bwd_fused(dev):
    import vit_amd.functional as vf

    x, g, b = randn((64, 64), dev, 25), randn((64,), dev, 26), randn((64,), dev, 27)
    _, mean, rstd = vf.layernorm_fwd(x, g, b, 1e-12, out_dtype=torch.float32)
    dy, dres = randn((64, 64), dev, 28, torch.bfloat16), randn((64, 64), dev, 29)
    E = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)
    return lambda: list(vf.layernorm_bwd_fused(dy, x, g, mean, rstd, dres, E(64, 64), E(64), E(64), E(64, 64, dt=torch.bfloat16),
                                               E(64), (0.1, 5, 6)))


def _colsum(dev):
    import vit_amd.functional as vf

    a = randn((1024, 768), dev, 30, torch.bfloat16)
    return lambda: [vf.colsum(a)]


def _colsum_rows(dev):
    import vit_amd.functional as vf

    a = randn((4, 256), dev, 31, torch.bfloat16)
    return lambda: [vf.colsum_rows(a, torch.empty(256, device=dev), row_stride=64, full_rows=256)]


def _linear_bwd_dw_rows(dev):
    import vit_amd.functional as vf

    dy, x = randn((4, 128), dev, 32), randn((4, 128), dev, 33)
    return lambda: [vf.linear_bwd_dw_rows(dy, x, torch.empty((128, 128), device=dev), row_stride=64, full_rows=256)]


def _cov_accumulate(dev):
    import vit_amd.functional as vf

    x, mu = randn((300, 200), dev, 34), randn((200,), dev, 35)
    return lambda: [vf.cov_accumulate(x, mu, torch.zeros((200, 200), device=dev))]


def _embed_finish_bwd(dev):
    import vit_amd.functional as vf

    dtok = randn((4, 9, 64), dev, 36)

    def run():
        dcls, dpos = torch.empty(64, device=dev), torch.empty((9, 64), device=dev)
        return [vf.embed_finish_bwd(dtok, dcls, dpos, dropout=(0.1, 7, 0)), dcls, dpos]
    return run


def _head_loss_bwd(dev):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    last, W, b = randn((4, 9, 64), dev, 37), randn((3, 64), dev, 38), randn((3,), dev, 39)
    labels, dloss = randn((4, 3), dev, 40), torch.ones((), device=dev)
    logits, _ = vf.head_loss_fwd(last, W, b, labels, _cabi.LOSS_MSE)
    return lambda: list(vf.head_loss_bwd(last, W, logits, labels, dloss, _cabi.LOSS_MSE))


def _grad_sqnorm(dev):
    import vit_amd.functional as vf

    g = randn((4096,), dev, 41)
    return lambda: [vf.grad_sqnorm(g)]


WRAPPED = {
    "gemm_splitk_dw": _gemm_dw,
    "gemm_colsum_pingpong": lambda dev: _gemm_colsum(dev, 512, 256, 256),
    "gemm_colsum_generic": lambda dev: _gemm_colsum(dev, 200, 64, 64),
    "attention_bwd_pipelined": lambda dev: _attention_bwd(dev, 2, 4, 65, 64),
    "attention_bwd_resident": lambda dev: _attention_bwd(dev, 2, 4, 65, 32),
    "attention_bwd_tiled": lambda dev: _attention_bwd(dev, 1, 2, 600, 64),
    "layernorm_bwd_fused": _layernorm_bwd_fused,
    "colsum": _colsum,
    "colsum_rows": _colsum_rows,
    "linear_bwd_dw_rows_f32": _linear_bwd_dw_rows,
    "cov_accumulate": _cov_accumulate,
    "embed_finish_bwd": _embed_finish_bwd,
    "head_loss_bwd": _head_loss_bwd,
    "grad_sqnorm": _grad_sqnorm,
}


@pytest.mark.parametrize("name", list(WRAPPED))
def test_same_bits_whatever_the_workspace_was(dev, name):
    import vit_amd.functional as vf

    run = WRAPPED[name](dev)
    small, default = handle(dev, 0), handle(dev)
    with vf.use_handle(small):
        got = run()
    needed = small.lib.vit_workspace_needed()  # of the call that was refused on the empty workspace, then repeated
    assert 0 < needed <= small.workspace_bytes, (needed, small.workspace_bytes)
    with vf.use_handle(default):
        want = run()
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), (name, i)


# ---------------------------------------------------------------------------------- (c) a retry does not add twice
def test_retry_under_grad_accumulate_adds_once(dev):
    import vit_amd.functional as vf

    dy, x = randn((4096, 256), dev, 51, torch.bfloat16), randn((4096, 256), dev, 52, torch.bfloat16)
    a, b = randn((1024, 128), dev, 53, torch.bfloat16), randn((1024, 128), dev, 54, torch.bfloat16)
    old_w, old_c, old_cs = randn((256, 256), dev, 55), randn((128, 128), dev, 56), randn((128,), dev, 57)

    def run(h):
        with vf.use_handle(h):
            dW = vf.linear_bwd_dw(dy, x, out=old_w.clone())
            cs = old_cs.clone()
            c = vf.gemm(a, b, M=128, N=128, K=1024, a_trans=True, b_trans=True, out=old_c.clone(), split_k=-1, colsum_out=cs)
        return dW, c, cs

    got = run(handle(dev, 0, grad_accumulate=1))
    want = run(handle(dev, grad_accumulate=1))
    new = run(handle(dev))  # overwrite mode: `new` itself
    torch.cuda.synchronize()
    for g, w, o, n in zip(got, want, (old_w, old_c, old_cs), new):
        assert torch.equal(g, w)
        assert torch.equal(w, o + n)  # old + new, one f32 add


# ---------------------------------------------------------------------------------- (d) the engine does not care
@pytest.mark.parametrize("precision", ["bf16-mixed", "32"])
def test_engine_on_an_empty_workspace(dev, precision):
    from test_cls_tail_gpu import build, case, hip_pass

    rc, sd, flux, labels, _, _ = case("l1")
    x, y = flux.to(dev), labels.to(dev)
    grads = []
    for empty in (False, True):
        model = build(rc, sd, dev, precision)
        eng = model.engine
        if empty:
            eng._main_handle = handle(dev, 0, reserve_cus=eng.reserve_cus)
        hip_pass(model, x, y, True, tail=True)
        torch.cuda.synchronize()
        grads.append(eng.grads.detach().clone())
        if empty:
            assert eng._main_handle.workspace_bytes > 0
    assert torch.equal(grads[0], grads[1])


# ---------------------------------------------------------------------------------- (e) vit_gemm's exact claim is a sufficient one
GUARD = 1 << 16  # sentinel bytes behind the workspace
GUARD_BYTE = 0xA5


def real_gemm_desc(dev, kw):
    """The descriptor of tests/test_workspace_cpu.py's gemm_desc over real tensors: inputs seeded by their name, outputs filled
    with SENTINEL (an accumulating C reads it as its old value).  Returns (descriptor, {name: tensor})."""
    from test_workspace_cpu import BF16, gemm_desc

    held = {}

    def buf(name, rows, cols, dtype):
        tdt = torch.bfloat16 if dtype == BF16 else torch.float32
        if name in ("C", "colsum_out", "aux_out"):
            t = filled((rows, cols), dev, tdt)
        elif name in ("rope_cos", "rope_sin"):  # the reference's table: angle t * theta_i
            ang = torch.arange(rows, dtype=torch.float32)[:, None] * 10000.0 ** (-torch.arange(cols, dtype=torch.float32) / cols)
            t = (ang.cos() if name == "rope_cos" else ang.sin()).to(dev)
        else:
            t = randn((rows, cols), dev, 60 + sum(map(ord, name)), tdt)
        held[name] = t
        return t.data_ptr()

    return gemm_desc(**kw, buf=buf), held


def gemm_on_exact_workspace(dev, kw, need, **options):
    """Refused on an empty workspace (where it needs one), then run on exactly vit_workspace_needed() bytes with sentinel bytes
    behind them, then on a large one: returns the outputs of the exact and of the large run."""
    import vit_amd.functional as vf

    h = handle(dev, 0, **options)
    lib, st = h.lib, vf._stream(torch.empty(1, device=dev))
    d, held = real_gemm_desc(dev, kw)
    rc = lib.vit_gemm(h.h, ctypes.byref(d), st)
    if need:
        assert rc == WS, (rc, lib.vit_last_error())
        assert lib.vit_workspace_needed() == need
        assert untouched(*(t for name, t in held.items() if name in ("C", "colsum_out", "aux_out")))
        big = torch.full((need + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        assert lib.vit_set_workspace(h.h, big.data_ptr(), need) == 0
        rc = lib.vit_gemm(h.h, ctypes.byref(d), st)
        torch.cuda.synchronize()
        assert bool((big[need:] == GUARD_BYTE).all())
    assert rc == 0, (rc, lib.vit_last_error())
    large = handle(dev, 8 << 20, **options)
    d2, held2 = real_gemm_desc(dev, kw)
    assert lib.vit_gemm(large.h, ctypes.byref(d2), st) == 0, lib.vit_last_error()
    torch.cuda.synchronize()
    return held, held2


def _gemm_table():
    from test_workspace_cpu import GEMM_TABLE

    return GEMM_TABLE


@pytest.mark.parametrize("name", list(_gemm_table()))
def test_gemm_exact_claim_is_sufficient(dev, name):
    kw, need, symbol = _gemm_table()[name]
    exact, large = gemm_on_exact_workspace(dev, kw, need)
    assert _cabi_lib().vit_last_gemm_kernel().decode() == symbol
    for out in ("C", "colsum_out", "aux_out"):
        if out in exact:
            assert not untouched(exact[out]), out
            assert torch.equal(exact[out], large[out]), (name, out)


def _cabi_lib():
    from vit_amd import _cabi

    return _cabi.load()


# accumulate with colsum_out under grad_accumulate: the stages' front (split-K slabs: 4 x 128 x 128 x 4 bytes on the generic core,
# 8 x 256 x 256 x 4 on the ping-pong core; vit_colsum's partials are smaller) and the M x N scratch matrix behind it
@pytest.mark.parametrize("M,N,K,need", [(128, 128, 1024, 4 * 65536 + 65536), (256, 256, 4096, 8 * 262144 + 262144)])
def test_gemm_scratch_route_on_its_exact_claim_adds_once(dev, M, N, K, need):
    kw = dict(M=M, N=N, K=K, a_trans=1, b_trans=1, split_k=-1, colsum=True)
    exact, large = gemm_on_exact_workspace(dev, kw, need, grad_accumulate=1)  # refused once, then repeated
    new, _ = gemm_on_exact_workspace(dev, kw, need - M * N * 4)  # overwrite mode: `new` itself, no scratch matrix
    for out in ("C", "colsum_out"):
        assert torch.equal(exact[out], large[out]), out
        assert torch.equal(exact[out], SENTINEL + new[out]), out  # old + new, one f32 add
