"""Every kernel call over poisoned outputs and a poisoned workspace (tests/_poison.py): each case runs one entry point twice, over
0xFF (NaN) and 0x7F (3.39e38) fills of everything it may write or use as scratch, demands finite, bit-identical results and
untouched pad regions, and then compares the result with a plain PyTorch reference at the tolerance tests/test_kernels_gpu.py
asserts for that kernel and dtype (exact where that test is exact).

Workspace words: every ctx_claim in vit_amd/csrc hands out floating-point scratch only (split-K slabs, partial rows, dz, row
losses, norm partials in f64, covariance slabs); no kernel keeps an index, counter or flag there, and there are no atomics.
LAMB's 16-byte header holds the one f32 trust ratio of the by-value form, written by lamb_ratio_kernel before lamb_apply_kernel
reads it.  So every entry point's workspace is poisoned; none is left out.

CASES is the table; tests/test_poison_cpu.py checks that every exported vit_* name is a case's entry point or in EXEMPT."""
import functools
import math
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _poison import IntOut, poisoned

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
Case = namedtuple("Case", "id entries fn")
CASES = []

# exported names no case calls, each with the reason in one line
EXEMPT = {
    "vit_version": "no output",
    "vit_last_error": "no output",
    "vit_create": "set-up only",
    "vit_destroy": "set-up only",
    "vit_set_workspace": "set-up only",
    "vit_workspace_needed": "no output",
    "vit_set_option": "set-up only",
    "vit_handle_set_option": "set-up only",
    "vit_step_state_bind": "set-up only",
    "vit_step_advance": "in place",
    "vit_last_gemm_kernel": "no output",
    "vit_embed_finish": "in place",
    "vit_embed_finish_gather": "in place",
    "vit_grad_sqnorm_acc": "accumulates by contract",
    "vit_optim_groups_write": "set-up only: writes a table from kernel arguments",
    "vit_layer_scale_table_write": "set-up only: writes a table from kernel arguments",
    "vit_mix_plan_write": "set-up only: writes a table from kernel arguments",
    "vit_ema_update": "in place",
}


def add(cid, entries, fn):
    CASES.append(Case(cid, (entries,) if isinstance(entries, str) else tuple(entries), fn))


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-20))


def bf(t):
    return t.to(BF16)


def randn(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


def E(dev, *s, dt=F32):
    return torch.empty(s, dtype=dt, device=dev)


def dn(dt):
    return "bf16" if dt == BF16 else "f32"


class option:
    """A process-wide kernel-selection option for the block, restored in `finally` fashion."""

    def __init__(self, name, value, default):
        self.name, self.value, self.default = name, value, default

    def __enter__(self):
        from vit_amd import _cabi

        _cabi.set_option(self.name, self.value)

    def __exit__(self, *exc):
        from vit_amd import _cabi

        _cabi.set_option(self.name, self.default)
        return False


class nothing:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_reserved = {}


def reserved(dev):
    """use_handle(a handle of its own with reserve_cus = 8): the one-workgroup-per-CU kernels launch fewer workgroups."""
    import vit_amd.functional as vf
    from vit_amd import _cabi

    idx = dev.index or 0
    if idx not in _reserved:
        _reserved[idx] = _cabi.Handle(idx, workspace_bytes=64 << 20)
        _reserved[idx].set_option("reserve_cus", 8)
    return vf.use_handle(_reserved[idx])


# =================================================================================================== GEMM
def gemm_tol(ab, cdt):
    return 3e-5 if ab == F32 else 2e-5 if cdt == F32 else 4e-3


def gemm_plain(dev, M, N, K, layout, cdt, ab=BF16, core=None, split_k=0, strided=False, reserve=False):
    import vit_amd.functional as vf

    a_t, b_t = layout in ("tn", "tt"), layout in ("nn", "tn")
    if a_t and M % 8:
        pytest.skip("transposed A needs M % 8 == 0")
    pad = 8 if strided else 0
    A, Bm = randn((M, K), dev, 1).to(ab), randn((N, K), dev, 2).to(ab)
    ref = A.double() @ Bm.double().t()

    def store(t, tr):  # the operand as the layout stores it, inside a wider tensor when strided
        t = t.t() if tr else t
        wide = randn((t.shape[0], t.shape[1] + pad), dev, 3).to(ab)
        wide[:, :t.shape[1]] = t
        return wide

    a_s, b_s = store(A, a_t), store(Bm, b_t)
    buf = E(dev, M, N + pad, dt=cdt)
    out, pads = buf[:, :N], ([buf[:, N:]] if pad else [])

    def run():
        vf.gemm(a_s, b_s, M=M, N=N, K=K, a_trans=a_t, b_trans=b_t, lda=a_s.shape[1], ldb=b_s.shape[1], out=buf, ldc=N + pad,
                split_k=split_k)

    with option("gemm_core", core, 1) if core is not None else nothing(), reserved(dev) if reserve else nothing():
        got, = poisoned(dev, run, [out], pads)
    e = rel(got, ref)
    print(f"gemm {M}x{N}x{K} {layout} rel {e:.3e}")
    assert e < gemm_tol(ab, cdt), e


for cdt in (BF16, F32):
    for lay in ("nt", "nn", "tn", "tt"):
        add(f"gemm generic (104, 40, 72) {lay} {dn(cdt)}", "vit_gemm", functools.partial(gemm_plain, M=104, N=40, K=72, layout=lay, cdt=cdt))
        add(f"gemm generic (320, 192, 192) {lay} {dn(cdt)}", "vit_gemm",
            functools.partial(gemm_plain, M=320, N=192, K=192, layout=lay, cdt=cdt, core=0))
    add(f"gemm strided (104, 40, 72) nt {dn(cdt)}", "vit_gemm",
        functools.partial(gemm_plain, M=104, N=40, K=72, layout="nt", cdt=cdt, strided=True))
    add(f"gemm strided (320, 192, 192) nn {dn(cdt)}", "vit_gemm",
        functools.partial(gemm_plain, M=320, N=192, K=192, layout="nn", cdt=cdt, strided=True))
for sk in (2, 5, 64, -1):
    add(f"gemm split_k={sk} (96, 64, 1024)", "vit_gemm", functools.partial(gemm_plain, M=96, N=64, K=1024, layout="nt", cdt=F32, split_k=sk))
for (M, N, K), lay, sk in (((104, 40, 72), "nt", 0), ((104, 40, 72), "tn", 0), ((320, 192, 192), "nn", 0), ((320, 192, 192), "nn", -1),
                           ((104, 40, 72), "nt", -1)):
    add(f"gemm x3 ({M}, {N}, {K}) {lay} split_k={sk}", "vit_gemm",
        functools.partial(gemm_plain, M=M, N=N, K=K, layout=lay, cdt=F32, ab=F32, split_k=sk))
for (M, N, K) in ((256, 256, 64), (512, 512, 192)):
    for lay in ("nt", "nn", "tn"):
        for cdt in (BF16, F32):
            add(f"gemm ping-pong ({M}, {N}, {K}) {lay} {dn(cdt)}", "vit_gemm",
                functools.partial(gemm_plain, M=M, N=N, K=K, layout=lay, cdt=cdt, core=5))
add("gemm ping-pong (512, 256, 128) split_k=-1", "vit_gemm",
    functools.partial(gemm_plain, M=512, N=256, K=128, layout="tn", cdt=F32, core=5, split_k=-1))
add("gemm ping-pong (512, 256, 128) nt split_k=-1", "vit_gemm",
    functools.partial(gemm_plain, M=512, N=256, K=128, layout="nt", cdt=F32, core=5, split_k=-1))
for res in (False, True):
    for cdt in (BF16, F32):
        add(f"gemm ping-pong many tiles (9472, 768, 64) {dn(cdt)}" + (" reserve_cus=8" if res else ""), "vit_gemm",
            functools.partial(gemm_plain, M=256 * 37, N=768, K=64, layout="nt", cdt=cdt, reserve=res))


def gemm_epilogues(dev, which, ab=BF16):
    """The fused epilogues of tests/test_kernels_gpu.py::test_gemm_epilogues at its shape, one per case."""
    import vit_amd.functional as vf
    from vit_amd._cabi import ACT_GELU, ACT_GELU_GRAD, ACT_MUL_AUX

    M, N, K = 330, 256, 192
    x, W = randn((M, K), dev, 3).to(ab), randn((N, K), dev, 4, 0.1).to(ab)
    bias, res = randn((N,), dev, 5), randn((M, N), dev, 6)
    base = x.double() @ W.double().t() + bias.double()
    if which == "gelu_aux":
        y, aux = E(dev, M, N, dt=BF16), E(dev, M, N, dt=BF16)
        y, aux = poisoned(dev, lambda: vf.linear_fwd(x, W, bias, act=ACT_GELU, aux_out=aux, out=y), [y, aux])
        assert rel(aux, base) < 4e-3 and rel(y, F.gelu(base)) < 5e-3
    elif which == "gelu_grad_mul_aux":
        dy, W2 = bf(randn((M, K), dev, 123)), bf(randn((K, N), dev, 124, 0.1))
        y, aux, dU = (E(dev, M, N, dt=BF16) for _ in range(3))

        def run():
            vf.gemm(x, W, M=M, N=N, K=K, bias=bias, act=ACT_GELU_GRAD, aux_out=aux, out=y)
            vf.gemm(dy, W2, M=M, N=N, K=K, b_trans=True, act=ACT_MUL_AUX, aux_in=aux, out=dU)

        y, aux, dU = poisoned(dev, run, [y, aux, dU])
        pre = base.clone().requires_grad_(True)
        ref = F.gelu(pre)
        ref.backward(dy.double() @ W2.double())
        gp = torch.autograd.grad(F.gelu(pre).sum(), pre)[0]
        assert rel(y, ref.detach()) < 6e-3 and rel(aux, gp) < 4e-3 and rel(dU, pre.grad) < 8e-3
    elif which == "residual_f32":
        y = E(dev, M, N)
        y, = poisoned(dev, lambda: vf.linear_fwd(x, W, bias, residual=res, out=y), [y])
        assert rel(y, base + res) < 2e-5
    elif which == "dropout":
        drop = (0.1, 77, 5)
        y = E(dev, M, N)
        y, = poisoned(dev, lambda: vf.linear_fwd(x, W, bias, dropout=drop, residual=res, out=y), [y])
        mask = vf.dropout_bwd_cast(torch.ones((M, N), device=dev), drop).float()
        assert rel(y, base * mask + res) < 5e-3  # mask scale is bf16-rounded in this reconstruction
        assert ((y - res != 0) == (mask != 0)).float().mean() > 0.999
    elif which == "dgelu":
        dy, u = randn((M, N), dev, 7).to(ab), randn((M, K), dev, 8).to(ab)
        dx = E(dev, M, K)
        dx, = poisoned(dev, lambda: vf.linear_bwd_dx(dy, W, dgelu_aux=u, out=dx), [dx])
        uu = u.double().requires_grad_(True)
        F.gelu(uu).backward(dy.double() @ W.double())
        assert rel(dx, uu.grad) < gemm_tol(ab, F32)
    elif which == "row_map":
        Bn, rpb = 6, 55
        xx = bf(randn((Bn * rpb, K), dev, 9))
        buf = E(dev, Bn * (rpb + 1), N)
        o3 = buf.view(Bn, rpb + 1, N)
        got, = poisoned(dev, lambda: vf.gemm(xx, W, M=Bn * rpb, N=N, K=K, out=buf, bias=bias, row_map=(rpb, rpb + 1, 1)),
                        [o3[:, 1:]], [o3[:, 0]])
        assert rel(got, (xx.double() @ W.double().t() + bias.double()).view(Bn, rpb, N)) < 2e-5
    elif which == "colsum_out":
        out, cs = E(dev, M, N, dt=BF16), E(dev, N)
        out, cs = poisoned(dev, lambda: vf.gemm(x, W, M=M, N=N, K=K, out=out, colsum_out=cs), [out, cs])
        assert rel(out, base - bias.double()) < 4e-3 and rel(cs, out.double().sum(0)) < 1e-5
    elif which == "dw":
        dy = randn((M, N), dev, 7).to(ab)
        dw = E(dev, N, K)
        dw, = poisoned(dev, lambda: vf.linear_bwd_dw(dy, x, out=dw), [dw])
        assert rel(dw, dy.double().t() @ x.double()) < gemm_tol(ab, F32)
    else:
        raise AssertionError(which)


for which in ("gelu_aux", "gelu_grad_mul_aux", "residual_f32", "dropout", "dgelu", "row_map", "colsum_out", "dw"):
    add(f"gemm epilogue {which} (330, 256, 192)", "vit_gemm", functools.partial(gemm_epilogues, which=which))
add("gemm x3 epilogue dgelu (330, 256, 192)", "vit_gemm", functools.partial(gemm_epilogues, which="dgelu", ab=F32))
add("gemm x3 epilogue dw (330, 256, 192)", "vit_gemm", functools.partial(gemm_epilogues, which="dw", ab=F32))


def gemm_pp_colsum(dev, dgelu, reserve):
    """colsum_out riding in the ping-pong epilogue: tiles_m * 2 partial rows in the workspace."""
    import vit_amd.functional as vf
    from vit_amd._cabi import ACT_DGELU, ACT_NONE

    M, N, K = 256 * 5, 768, 256
    dy, W, u = bf(randn((M, K), dev, 110)), bf(randn((K, N), dev, 111, 0.1)), bf(randn((M, N), dev, 112))
    out, cs = E(dev, M, N, dt=BF16), E(dev, N)

    def run():
        vf.gemm(dy, W, M=M, N=N, K=K, b_trans=True, act=ACT_DGELU if dgelu else ACT_NONE, aux_in=u if dgelu else None, out=out,
                colsum_out=cs)

    with reserved(dev) if reserve else nothing():
        out, cs = poisoned(dev, run, [out, cs])
    ref = dy.double() @ W.double()
    if dgelu:
        uu = u.double().requires_grad_(True)
        F.gelu(uu).backward(ref)
        ref = uu.grad
    assert rel(out, ref) < 4e-3 and rel(cs, out.double().sum(0)) < 1e-5


for dg in (False, True):
    for res in (False, True):
        add(f"gemm ping-pong colsum_out (1280, 768, 256) nn{' dgelu' if dg else ''}{' reserve_cus=8' if res else ''}", "vit_gemm",
            functools.partial(gemm_pp_colsum, dgelu=dg, reserve=res))


def rope_ref(y, cos, sin, T, H, dh):
    """fp64 rotate-half rotation of columns [0, 2 * H * dh) of y, position = row % T (test_gemm_rope_epilogue's reference)."""
    M, D = y.shape[0], H * dh
    t = torch.arange(M, device=y.device) % T
    c, s = cos.double()[t], sin.double()[t]
    ref = y.clone()
    for part in range(2):
        blk = y[:, part * D:(part + 1) * D].view(M, H, dh)
        x1, x2 = blk[..., : dh // 2], blk[..., dh // 2:]
        rot = torch.cat([x1 * c[:, None] - x2 * s[:, None], x2 * c[:, None] + x1 * s[:, None]], -1)
        ref[:, part * D:(part + 1) * D] = rot.reshape(M, D)
    return ref


def gemm_rope(dev, M, K, H, dh, T, ncols, core=None, fused=None):
    """vit_gemm with the rope descriptor; ncols = 2: a Q / K-only projection, N = rope_cols = 2 * H * dh (legal by gemm_plan; the
    pass behind the product used to refuse its ld after the product was written)."""
    import vit_amd.functional as vf
    from vit_amd import _cabi

    D = H * dh
    N = ncols * D
    x, W, bias = bf(randn((M, K), dev, 300, 0.5)), bf(randn((N, K), dev, 301, 0.1)), randn((N,), dev, 302)
    inv = 1.0 / (10000.0 ** (torch.arange(0, dh, 2).float() / dh))
    fr = torch.outer(torch.arange(T).float(), inv)
    cos, sin = fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)
    out = E(dev, M, N, dt=BF16)
    with option("gemm_core", core, 1) if core is not None else nothing():
        got, = poisoned(dev, lambda: vf.gemm(x, W, M=M, N=N, K=K, bias=bias, out=out, rope=(cos, sin, T, dh, 2 * D)), [out])
        sym = _cabi.load().vit_last_gemm_kernel().decode()
    if fused is not None:
        assert ("<0, 0, 8, 8>" in sym) == fused, sym
    ref = rope_ref(x.double() @ W.double().t() + bias.double(), cos, sin, T, H, dh)
    assert rel(got, ref) < 4e-3, rel(got, ref)


add("gemm rope q/k only (104, 64, 72) generic", ("vit_gemm", "vit_rope_qk"), functools.partial(gemm_rope, M=104, K=72, H=2, dh=16, T=13, ncols=2))
add("gemm rope q/k only (256, 256, 64) ping-pong fused", "vit_gemm",
    functools.partial(gemm_rope, M=256, K=64, H=2, dh=64, T=32, ncols=2, core=5, fused=True))
add("gemm rope q/k only (256, 256, 64) ping-pong pass behind", ("vit_gemm", "vit_rope_qk"),
    functools.partial(gemm_rope, M=256, K=64, H=1, dh=128, T=32, ncols=2, core=5, fused=False))
add("gemm rope (1024, 768, 64) ping-pong rotating epilogue", "vit_gemm",
    functools.partial(gemm_rope, M=1024, K=64, H=4, dh=64, T=197, ncols=3, fused=True))


def linear_exports(dev, which):
    """The three convenience exports themselves (vit_amd.functional reaches the same kernels through vit_gemm)."""
    import vit_amd.functional as vf
    from _poison import active_handle
    from vit_amd._cabi import ACT_NONE, VIT_BF16, VIT_F32

    M, N, K = 104, 40, 72
    x, W, dy = bf(randn((M, K), dev, 3)), bf(randn((N, K), dev, 4, 0.1)), bf(randn((M, N), dev, 7))
    bias = randn((N,), dev, 5)
    h, st = active_handle(dev), vf._stream(x)
    if which == "fwd":
        y = E(dev, M, N, dt=BF16)
        y, = poisoned(dev, lambda: h.call("vit_linear_fwd", x.data_ptr(), W.data_ptr(), bias.data_ptr(), y.data_ptr(), VIT_BF16, M, N, K,
                                          ACT_NONE, None, 0.0, 0, 0, None, st), [y])
        assert rel(y, x.double() @ W.double().t() + bias.double()) < 4e-3
    elif which == "bwd_dx":
        dx = E(dev, M, K)
        dx, = poisoned(dev, lambda: h.call("vit_linear_bwd_dx", dy.data_ptr(), W.data_ptr(), dx.data_ptr(), VIT_F32, M, N, K, None, st), [dx])
        assert rel(dx, dy.double() @ W.double()) < 2e-5
    else:
        dw = E(dev, N, K)
        dw, = poisoned(dev, lambda: h.call("vit_linear_bwd_dw", dy.data_ptr(), x.data_ptr(), dw.data_ptr(), M, N, K, 0, st), [dw])
        assert rel(dw, dy.double().t() @ x.double()) < 2e-5


for which in ("fwd", "bwd_dx", "bwd_dw"):
    add(f"vit_linear_{which} (104, 40, 72)", f"vit_linear_{which}", functools.partial(linear_exports, which=which))


# =================================================================================================== LayerNorm
EPS = 1e-12


def affine(D, dev):
    return randn((D,), dev, 21) * 0.1 + 1, randn((D,), dev, 22) * 0.1


def ln_fwd(dev, rows, D, odt):
    import vit_amd.functional as vf

    x = randn((rows, D), dev, 20) * 3 + 0.5
    g, b = affine(D, dev)
    y, mean, rstd = E(dev, rows, D, dt=odt), E(dev, rows), E(dev, rows)
    y, mean, rstd = poisoned(dev, lambda: vf.layernorm_fwd(x, g, b, EPS, out=y, mean=mean, rstd=rstd), [y, mean, rstd])
    assert rel(y, F.layer_norm(x, (D,), g, b, EPS)) < (1e-6 if odt == F32 else 4e-3)
    assert rel(mean, x.mean(-1)) < 1e-6


for rows, D in ((5, 36), (516, 32), (320, 192), (77, 1024), (33, 2048)):
    for odt in (BF16, F32):
        add(f"vit_layernorm_fwd ({rows}, {D}) {dn(odt)}", "vit_layernorm_fwd", functools.partial(ln_fwd, rows=rows, D=D, odt=odt))


def ln_fwd_residual(dev, rows, D, ddt, stride=1):
    import vit_amd.functional as vf

    x = randn((rows * stride, D), dev, 90) * 2 + 0.3
    delta = randn((rows, D), dev, 91).to(ddt)
    g, b = affine(D, dev)
    ref_sum = x[::stride] + delta.float()
    for odt in (BF16, F32):
        xs, y, mean, rstd = E(dev, rows, D), E(dev, rows, D, dt=odt), E(dev, rows), E(dev, rows)
        xs, y, mean, rstd = poisoned(dev, lambda: vf.layernorm_fwd_residual(x, delta, xs, g, b, EPS, out=y, mean=mean, rstd=rstd,
                                                                            x_row_stride=stride), [xs, y, mean, rstd])
        assert torch.equal(xs, ref_sum)
        assert rel(y, F.layer_norm(ref_sum, (D,), g, b, EPS)) < (1e-6 if odt == F32 else 4e-3)
        assert rel(mean, ref_sum.mean(-1)) < 1e-6


for rows, D in ((37, 32), (129, 1024)):
    for ddt in (BF16, F32):
        add(f"vit_layernorm_fwd_residual ({rows}, {D}) delta {dn(ddt)}", "vit_layernorm_fwd_residual",
            functools.partial(ln_fwd_residual, rows=rows, D=D, ddt=ddt))
add("vit_layernorm_fwd_residual_rows x_row_stride=17 (6, 192)", "vit_layernorm_fwd_residual_rows",
    functools.partial(ln_fwd_residual, rows=6, D=192, ddt=BF16, stride=17))


def ln_bwd_ref(x, g, b, dy):
    xx, gg, bb = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    F.layer_norm(xx, (x.shape[-1],), gg, bb, EPS).backward(dy.float())
    return xx.grad, gg.grad, bb.grad


def ln_stats(x, g, b):
    import vit_amd.functional as vf

    _, mean, rstd = vf.layernorm_fwd(x, g, b, EPS, out_dtype=F32)
    return mean, rstd


def ln_bwd(dev, rows, D, with_dres, dydt=F32):
    import vit_amd.functional as vf

    x = randn((rows, D), dev, 20) * 3 + 0.5
    g, b = affine(D, dev)
    mean, rstd = ln_stats(x, g, b)
    dy, dres = randn((rows, D), dev, 23).to(dydt), randn((rows, D), dev, 24) if with_dres else None
    dx, dg, db = E(dev, rows, D), E(dev, D), E(dev, D)
    dx, dg, db = poisoned(dev, lambda: vf.layernorm_bwd(dy, x, g, mean, rstd, dres=dres, dx=dx, dgamma=dg, dbeta=db), [dx, dg, db])
    rx, rg, rb = ln_bwd_ref(x, g, b, dy)
    assert rel(dx, rx + dres if with_dres else rx) < 1e-5 and rel(dg, rg) < 1e-5 and rel(db, rb) < 1e-5


for rows, D in ((516, 32), (77, 1024), (33, 2048), (4112, 32)):
    add(f"vit_layernorm_bwd ({rows}, {D}) dres", "vit_layernorm_bwd", functools.partial(ln_bwd, rows=rows, D=D, with_dres=True))
    add(f"vit_layernorm_bwd ({rows}, {D}) bf16 dy, no dres", "vit_layernorm_bwd",
        functools.partial(ln_bwd, rows=rows, D=D, with_dres=False, dydt=BF16))


def drop_mult(drop, rows, D, dev):
    """The dropout multiplier of every element of a [rows, D] tensor, restated on the host (oracle/dropmask.py)."""
    from oracle import dropmask as dm

    return torch.from_numpy(dm.multiplier(dm.drop_cfg(*drop), rows, D)).to(dev)


def ln_bwd_fused(dev, rows, D, drop, ndt):
    import vit_amd.functional as vf

    x = randn((rows, D), dev, 80) * 2 + 0.3
    g, b = affine(D, dev)
    mean, rstd = ln_stats(x, g, b)
    dy, dres = bf(randn((rows, D), dev, 83)), randn((rows, D), dev, 84)
    dx, dg, db, dyn, dbias = E(dev, rows, D), E(dev, D), E(dev, D), E(dev, rows, D, dt=ndt), E(dev, D)
    dx, dg, db, dyn, dbias = poisoned(dev, lambda: vf.layernorm_bwd_fused(dy, x, g, mean, rstd, dres, dx, dg, db, dyn, dbias, drop),
                                      [dx, dg, db, dyn, dbias])
    rx, rg, rb = ln_bwd_ref(x, g, b, dy)
    assert rel(dx, rx + dres) < 1e-5 and rel(dg, rg) < 1e-5 and rel(db, rb) < 1e-5
    assert torch.equal(dyn, (dx * drop_mult(drop, rows, D, dev)).to(ndt))
    assert rel(dbias, dyn.double().sum(0)) < 1e-5


for rows, D in ((516, 32), (77, 1024)):
    for drop in ((0.0, 0, 0), (0.1, 321, 9)):
        for ndt in (BF16, F32):
            add(f"vit_layernorm_bwd_fused ({rows}, {D}) p={drop[0]} dyn {dn(ndt)}", "vit_layernorm_bwd_fused",
                functools.partial(ln_bwd_fused, rows=rows, D=D, drop=drop, ndt=ndt))


def ln_bwd_rows(dev, form, fused):
    """row_stride = 17: the tensors hold rows 0, 17, .. of 102 compactly; dres_row_stride = 17: dres alone is compact."""
    import vit_amd.functional as vf

    full, s, D = 102, 17, 192
    held = full // s
    rows = held if form == "row_stride" else full
    x = randn((rows, D), dev, 80) * 2 + 0.3
    g, b = affine(D, dev)
    mean, rstd = ln_stats(x, g, b)
    dy = bf(randn((rows, D), dev, 83))
    dres = randn((held, D), dev, 84)
    drop = (0.1, 321, 9)
    dx, dg, db = E(dev, rows, D), E(dev, D), E(dev, D)
    dyn, dbias = (E(dev, rows, D, dt=BF16), E(dev, D)) if fused else (None, None)
    kw = dict(row_stride=s, full_rows=full) if form == "row_stride" else dict(dres_row_stride=s)
    outs = [dx, dg, db] + ([dyn, dbias] if fused else [])
    got = poisoned(dev, lambda: vf.layernorm_bwd_rows(dy, x, g, mean, rstd, dres, dx, dg, db, dyn=dyn, dbias=dbias, dropout=drop, **kw),
                   outs)
    rx, rg, rb = ln_bwd_ref(x, g, b, dy)
    if form == "row_stride":
        rx = rx + dres
    else:
        rx[::s] += dres
    assert rel(got[0], rx) < 1e-5 and rel(got[1], rg) < 1e-5 and rel(got[2], rb) < 1e-5
    if fused:
        k = drop_mult(drop, full, D, dev)
        k = k[::s] if form == "row_stride" else k
        assert torch.equal(got[3], (got[0] * k).to(BF16))
        assert rel(got[4], got[3].double().sum(0)) < 1e-5


for form in ("row_stride", "dres_row_stride"):
    for fused in (False, True):
        add(f"vit_layernorm_bwd_rows {form}=17 over 102 rows{' fused' if fused else ''}", "vit_layernorm_bwd_rows",
            functools.partial(ln_bwd_rows, form=form, fused=fused))

PATH_SITE = 4 + 4 * 5


def path_rows(p, B, T, br, dev):
    """(seed, float32 [B * T, 1] multiplier of every row): the first seed at which the branch keeps and drops a sample."""
    from test_droppath_cpu import path_multiplier

    for seed in range(1000, 2000):
        m = path_multiplier(p, seed, PATH_SITE, B)[:, br]
        if 0 < int((m != 0).sum()) < B:
            return seed, torch.from_numpy(np.repeat(m, T)).to(dev).view(-1, 1)
    raise AssertionError("no seed")


def ln_path_fwd(dev, ddt):
    import vit_amd.functional as vf

    B, T, D, p, br = 6, 17, 192, 0.5, 0
    rows = B * T
    seed, mrow = path_rows(p, B, T, br, dev)
    dropped = (mrow == 0).view(-1)
    x, delta = randn((rows, D), dev, 11), randn((rows, D), dev, 12).to(ddt)
    g, b = affine(D, dev)
    xs, y, mean, rstd = E(dev, rows, D), E(dev, rows, D, dt=BF16), E(dev, rows), E(dev, rows)
    xs, y, mean, rstd = poisoned(dev, lambda: vf.layernorm_fwd_residual_path(x, delta, xs, g, b, EPS, (p, PATH_SITE, T, br), seed, out=y,
                                                                             mean=mean, rstd=rstd), [xs, y, mean, rstd])
    ref_sum = torch.where(dropped.view(-1, 1), x, x + delta.float() * mrow)  # p = 0.5: the kept scale 2 is exact
    assert torch.equal(xs[dropped], x[dropped])  # a dropped sample's rows are still written: xsum = x there
    assert torch.equal(xs, ref_sum)
    assert rel(y, F.layer_norm(ref_sum, (D,), g, b, EPS)) < 4e-3 and rel(mean, ref_sum.mean(-1)) < 1e-6


def ln_path_bwd(dev, ph):
    import vit_amd.functional as vf

    B, T, D, p, br = 6, 17, 192, 0.5, 1
    rows = B * T
    seed, mrow = path_rows(p, B, T, br, dev)
    x = randn((rows, D), dev, 21)
    g, b = affine(D, dev)
    mean, rstd = ln_stats(x, g, b)
    dy, dres = bf(randn((rows, D), dev, 22)), randn((rows, D), dev, 23)
    drop = (ph, seed, 1 + 4 * 5 + 2)
    dx, dg, db, dyn, dbias = E(dev, rows, D), E(dev, D), E(dev, D), E(dev, rows, D, dt=BF16), E(dev, D)
    dx, dg, db, dyn, dbias = poisoned(
        dev, lambda: vf.layernorm_bwd_path(dy, x, g, mean, rstd, dres, dx, dg, db, dyn, dbias, (p, PATH_SITE, T, br), dropout=drop),
        [dx, dg, db, dyn, dbias])
    rx, rg, rb = ln_bwd_ref(x, g, b, dy)
    assert rel(dx, rx + dres) < 1e-5 and rel(dg, rg) < 1e-5 and rel(db, rb) < 1e-5
    k = drop_mult(drop, rows, D, dev) * mrow
    assert torch.equal(dyn, (dx * k).to(BF16))
    assert bool((dyn[(mrow == 0).view(-1)] == 0).all())  # a dropped sample's rows are written, as zeros
    assert rel(dbias, dyn.double().sum(0)) < 1e-5


for ddt in (BF16, F32):
    add(f"vit_layernorm_fwd_residual_path (102, 192) rows_per_sample=17 p=0.5 delta {dn(ddt)}", "vit_layernorm_fwd_residual_path",
        functools.partial(ln_path_fwd, ddt=ddt))
for ph in (0.0, 0.1):
    add(f"vit_layernorm_bwd_path (102, 192) rows_per_sample=17 p=0.5 dropout {ph}", "vit_layernorm_bwd_path",
        functools.partial(ln_path_bwd, ph=ph))


# =================================================================================================== attention
@functools.lru_cache(maxsize=None)
def attn_reference(dev, B, H, T, dh, drop, dt):
    """Inputs and the fp32 autograd reference of one (shape, dropout, dtype): computed once, shared by every option."""
    import vit_amd.functional as vf
    from test_kernels_gpu import attn_ref, extract_attn_mask

    scale = dh ** -0.5
    qkv = randn((B * T, 3 * H * dh), dev, 30).to(dt)
    dctx = randn((B * T, H * dh), dev, 31).to(dt)
    mask = None
    if drop[0]:
        mask = (extract_attn_mask(vf, dev, B, H, T, dh, drop) > 0.5).float() * (65536.0 / (65536 - round(drop[0] * 65536)))
    q32 = qkv.float().requires_grad_(True)
    ref, p, lse = attn_ref(q32, B, H, T, dh, scale, mask)
    ref.backward(dctx.float())
    return qkv, dctx, ref.detach(), p.detach(), lse.detach().reshape(B * H, T), q32.grad


def attention(dev, B, H, T, dh, drop, dt=BF16, split=2, fused=4, colsum=True, reserve=False):
    import vit_amd.functional as vf

    scale, D = dh ** -0.5, H * dh
    qkv, dctx, ref, p, lse_ref, g = attn_reference(dev, B, H, T, dh, drop, dt)
    ctx, lse, delta, dqkv = E(dev, B * T, D, dt=dt), E(dev, B * H, T), E(dev, B * H, T), E(dev, B * T, 3 * D, dt=dt)
    lo = E(dev, B * T, D, dt=dt) if dt == BF16 else None
    cs = E(dev, 3 * D) if colsum else None
    probs = E(dev, B, H, T, T) if not drop[0] else None  # vit_attention_probs has no dropout

    def run():
        vf.attention_fwd(qkv, B, H, T, dh, scale, dropout=drop, ctx=ctx, lse=lse, ctx_lo=lo)
        vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, scale, dropout=drop, dqkv=dqkv, delta=delta, colsum_out=cs, ctx_lo=lo)
        if probs is not None:
            vf.attention_probs(qkv, B, H, T, dh, scale, out=probs)

    named = {"ctx": ctx, "lse": lse, "delta": delta, "dqkv": dqkv, "ctx_lo": lo, "dqkv_colsum": cs, "probs": probs}
    names = [k for k, v in named.items() if v is not None]
    with option("attn_split", split, 2), option("attn_bwd_fused", fused, 4), reserved(dev) if reserve else nothing():
        got = dict(zip(names, poisoned(dev, run, [named[k] for k in names])))
    b16 = dt == BF16
    assert rel(got["ctx"], ref) < (6e-3 if b16 else 1e-5)
    assert rel(got["lse"], lse_ref) < (1e-5 if b16 else 1e-6)
    if probs is not None:
        assert rel(got["probs"], p) < 1e-5
    d, gg = got["dqkv"].float().view(B * T, 3, D), g.view(B * T, 3, D)
    if b16:
        for i, nm in enumerate("qkv"):
            assert rel(d[:, i], gg[:, i]) < 1.5e-2, (nm, rel(d[:, i], gg[:, i]))
    else:
        assert rel(d, gg) < 2e-5
    if colsum:
        assert rel(got["dqkv_colsum"], got["dqkv"].double().sum(0)) < 1e-5
    # delta = rowsum(dO * O) over each head, O = the stored context plus its stored rounding residual
    o = got["ctx"].double() + (got["ctx_lo"].double() if b16 else 0.0)
    dref = (dctx.double() * o).view(B, T, H, dh).sum(-1).permute(0, 2, 1).reshape(B * H, T)
    e = rel(got["delta"], dref)
    print(f"attention {(B, H, T, dh)} delta rel {e:.3e}")
    assert e < 1e-5, e


def _attn_id(shape, drop, dt, **kw):
    opts = "".join(f" {k}={v}" for k, v in kw.items())
    return f"attention {shape} {dn(dt)} p={drop[0]}{opts}"


ATT_DROP = ((0.0, 0, 0), (0.1, 9, 3))
ATT_ENTRIES = ("vit_attention_fwd", "vit_attention_bwd", "vit_attention_probs")
#            shape              resident  pair-pipelined kernel fits (head_dim 64, 64 <= T <= 208)
ATT_BF16 = (((2, 3, 5, 64), True, False), ((2, 2, 129, 16), True, False), ((1, 2, 197, 64), True, True), ((1, 2, 64, 64), True, True),
            ((1, 1, 640, 64), False, False), ((1, 2, 1025, 16), False, False), ((2, 8, 122, 4), True, False),
            ((300, 1, 100, 64), True, True), ((150, 2, 75, 64), True, True))
for shape, resident, pipelined in ATT_BF16:
    for drop in ATT_DROP:
        variants = [{}, {"colsum": False}, {"reserve": True}]
        if resident:
            variants.append({"split": 1})
        if pipelined:
            variants += [{"fused": 0}, {"fused": 0, "split": 1}]
        for kw in variants:
            add(_attn_id(shape, drop, BF16, **kw), ATT_ENTRIES,
                functools.partial(attention, B=shape[0], H=shape[1], T=shape[2], dh=shape[3], drop=drop, **kw))
for shape in ((2, 3, 5, 64), (1, 2, 197, 64), (2, 8, 122, 4), (1, 3, 130, 12)):
    for drop in ATT_DROP:
        for kw in ({}, {"colsum": False}):
            add(_attn_id(shape, drop, F32, **kw), ATT_ENTRIES,
                functools.partial(attention, B=shape[0], H=shape[1], T=shape[2], dh=shape[3], drop=drop, dt=F32, **kw))


# =================================================================================================== embedding side, elementwise
def unfold_cast(dev, odt):
    import vit_amd.functional as vf

    B, L, P, S = 3, 1000, 64, 48
    N = math.ceil((L - P) / S) + 1
    x = randn((B, L), dev, 40)
    out = E(dev, B * N, P, dt=odt)
    got, = poisoned(dev, lambda: vf.unfold_cast(x, P, S, N, out=out), [out])
    ref = x.unfold(1, P, S)
    assert ref.size(1) == N - 1  # the last window is ragged
    ref = torch.cat([ref, torch.zeros(B, 1, P, device=dev)], 1).reshape(B * N, P)
    assert torch.equal(got, ref.to(odt))
    assert bool((got.view(B, N, P)[:, -1] == 0).all())  # and comes out all zero


def fold_add(dev, L, P, S):
    import vit_amd.functional as vf

    B = 3
    N = math.ceil((L - P) / S) + 1
    dp = randn((B * N, P), dev, 45)
    out = E(dev, B, L)
    got, = poisoned(dev, lambda: vf.fold_add(dp, B, L, P, S, N, out=out), [out])
    x = torch.zeros((B, L), dtype=torch.float64, device=dev, requires_grad=True)
    u = x.unfold(1, P, S)
    u = torch.cat([u, torch.zeros(B, N - u.size(1), P, dtype=torch.float64, device=dev)], 1)
    u.backward(dp.double().view(B, N, P))
    assert rel(got, x.grad) < 1e-6, rel(got, x.grad)


for odt in (BF16, F32):
    add(f"vit_unfold_cast B=3 L=1000 P=64 S=48 {dn(odt)}", "vit_unfold_cast", functools.partial(unfold_cast, odt=odt))
add("vit_fold_add B=3 L=1000 P=64 S=48", "vit_fold_add", functools.partial(fold_add, L=1000, P=64, S=48))
add("vit_fold_add B=3 L=250 P=16 S=8", "vit_fold_add", functools.partial(fold_add, L=250, P=16, S=8))


def embed_finish_bwd(dev, B, T, D, p):
    import vit_amd.functional as vf

    drop = (p, 5, 1) if p else (0.0, 0, 0)
    dtok = randn((B, T, D), dev, 44)
    dpatch, dcls, dpos = E(dev, B * (T - 1), D, dt=BF16), E(dev, D), E(dev, T, D)
    dpatch, dcls, dpos = poisoned(dev, lambda: vf.embed_finish_bwd(dtok, dcls, dpos, dropout=drop, dpatch=dpatch), [dpatch, dcls, dpos])
    gm = dtok * drop_mult(drop, B * T, D, dev).view(B, T, D)
    assert rel(dcls, gm[:, 0].sum(0)) < 1e-6 and rel(dpos, gm.sum(0)) < 1e-6
    assert rel(dpatch, gm[:, 1:].reshape(B * (T - 1), D)) < 4e-3


for B, T, D in ((3, 129, 32), (20, 17, 64)):
    for p in (0.0, 0.1):
        add(f"vit_embed_finish_bwd ({B}, {T}, {D}) p={p}", "vit_embed_finish_bwd", functools.partial(embed_finish_bwd, B=B, T=T, D=D, p=p))


def dropout_bwd_cast(dev, rows, cols):
    import vit_amd.functional as vf

    dx = randn((rows, cols), dev, 50)
    for drop in ((0.0, 0, 0), (0.1, 7, 2)):
        for odt in (BF16, F32):
            out = E(dev, rows, cols, dt=odt)
            got, = poisoned(dev, lambda: vf.dropout_bwd_cast(dx, drop, out=out), [out])
            assert torch.equal(got, (dx * drop_mult(drop, rows, cols, dev)).to(odt))


for rows, cols in ((1000, 32), (77, 1028)):
    add(f"vit_dropout_bwd_cast ({rows}, {cols})", "vit_dropout_bwd_cast", functools.partial(dropout_bwd_cast, rows=rows, cols=cols))


def colsum(dev, rows, cols, dt, pad=0):
    import vit_amd.functional as vf

    a = randn((rows, cols + pad), dev, 50).to(dt)[:, :cols]
    out = E(dev, cols)
    got, = poisoned(dev, lambda: vf.colsum(a, out=out), [out])
    assert rel(got, a.double().sum(0)) < 1e-5, rel(got, a.double().sum(0))


for dt in (F32, BF16):
    add(f"vit_colsum (1234, 768) {dn(dt)}", "vit_colsum", functools.partial(colsum, rows=1234, cols=768, dt=dt))
add("vit_colsum (70000, 64) f32", "vit_colsum", functools.partial(colsum, rows=70000, cols=64, dt=F32))
add("vit_colsum (1234, 768) bf16 lda=cols+4", "vit_colsum", functools.partial(colsum, rows=1234, cols=768, dt=BF16, pad=4))


def rows_forms(dev, which, held, stride, cols, dt=BF16):
    """vit_colsum_rows / vit_linear_bwd_dw_rows: compact row j stands for row j * stride of a tensor of held * stride rows."""
    import vit_amd.functional as vf

    full = held * stride
    dy = randn((held, cols), dev, 32).to(dt)
    if which == "colsum_rows":
        out = E(dev, cols)
        got, = poisoned(dev, lambda: vf.colsum_rows(dy, out, row_stride=stride, full_rows=full), [out])
        assert rel(got, dy.double().sum(0)) < 1e-5
    else:
        K = 256 if cols % 256 == 0 else 64  # [256, 256] x 1024 rows: the full product would run the ping-pong core with split-K
        x = randn((held, K), dev, 33).to(dt)
        out = E(dev, cols, K)
        got, = poisoned(dev, lambda: vf.linear_bwd_dw_rows(dy, x, out, row_stride=stride, full_rows=full), [out])
        assert rel(got, dy.double().t() @ x.double()) < gemm_tol(dt, F32)


for which in ("colsum_rows", "linear_bwd_dw_rows"):
    add(f"vit_{which} ping-pong order full_rows=1024 row_stride=64 cols=256", f"vit_{which}",
        functools.partial(rows_forms, which=which, held=16, stride=64, cols=256))
    add(f"vit_{which} rows=6 row_stride=17 cols=192", f"vit_{which}", functools.partial(rows_forms, which=which, held=6, stride=17, cols=192))
    add(f"vit_{which} f32 full_rows=1024 row_stride=64 cols=256", f"vit_{which}",
        functools.partial(rows_forms, which=which, held=16, stride=64, cols=256, dt=F32))


def casts(dev, which):
    import vit_amd.functional as vf

    src = randn((1003,), dev, 51)
    if which == "f32_bf16":
        out = E(dev, 1003, dt=BF16)
        got, = poisoned(dev, lambda: vf.cast_f32_bf16(src, out=out), [out])
        assert torch.equal(got, bf(src))
    else:
        out = E(dev, 1003)
        got, = poisoned(dev, lambda: vf.cast_bf16_f32(bf(src), out, 0.5), [out])
        assert torch.equal(got, bf(src).float() * 0.5)


add("vit_cast_f32_bf16 n=1003", "vit_cast_f32_bf16", functools.partial(casts, which="f32_bf16"))
add("vit_cast_bf16_f32 n=1003 scale=0.5", "vit_cast_bf16_f32", functools.partial(casts, which="bf16_f32"))


def grad_sqnorm(dev):
    import vit_amd.functional as vf

    g = randn((1_000_003,), dev, 71, 0.01)
    out = E(dev, 1)
    sq, = poisoned(dev, lambda: vf.grad_sqnorm(g, out=out), [out])
    assert abs(sq.item() - float((g.double() ** 2).sum())) < 1e-4 * sq.item()


add("vit_grad_sqnorm n=1000003", "vit_grad_sqnorm", grad_sqnorm)


# =================================================================================================== head + loss
def head_loss(dev, kind, B, C):
    import vit_amd.functional as vf
    from vit_amd._cabi import LOSS_BCE, LOSS_CE, LOSS_L1, LOSS_MSE, LOSS_SOFT_CE

    T, D = 6, 192
    code = {"mse": LOSS_MSE, "l1": LOSS_L1, "ce": LOSS_CE, "soft_ce": LOSS_SOFT_CE, "bce": LOSS_BCE}[kind]
    last = randn((B, T, D), dev, 60)
    W, b = randn((C, D), dev, 61, 0.1), randn((C,), dev, 62, 0.1)
    gen = torch.Generator(device="cpu").manual_seed(63)
    if kind == "ce":
        labels = torch.randint(0, C, (B,), generator=gen).to(dev)
    elif kind == "soft_ce":
        labels = torch.rand((B, C), generator=gen).softmax(-1).to(dev)
    elif kind == "bce":
        labels = torch.rand((B, C), generator=gen).to(dev)
    else:
        labels = torch.rand((B, C) if C > 1 else (B,), generator=gen).to(dev)
    dloss = torch.full((1,), 1.7, device=dev)
    logits, loss, dlast, dW, db = E(dev, B, C), E(dev), E(dev, B, T, D), E(dev, C, D), E(dev, C)

    def run():
        vf.head_loss_fwd(last, W, b, labels, code, logits=logits, loss=loss)
        vf.head_loss_bwd(last, W, logits, labels, dloss, code, dlast=dlast, dW=dW, db=db)

    logits, loss, dlast, dW, db = poisoned(dev, run, [logits, loss, dlast, dW, db])
    l32 = last.clone().requires_grad_(True)
    W32, b32 = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lg = F.linear(l32[:, 0], W32, b32)
    if kind == "ce":
        ref = F.cross_entropy(lg, labels)
    elif kind == "l1":
        ref = F.l1_loss(lg.view(-1), labels.view(-1))
    elif kind == "mse":
        ref = F.mse_loss(lg.view(-1), labels.view(-1))
    elif kind == "soft_ce":
        ref = -(labels * lg.log_softmax(-1)).sum(-1).mean()
    else:
        ref = F.binary_cross_entropy_with_logits(lg, labels)
    assert rel(logits, lg) < 1e-5 and abs(loss.item() - ref.item()) < 1e-5 * max(1, abs(ref.item()))
    (ref * 1.7).backward()
    assert rel(dlast, l32.grad) < 1e-5 and rel(dW, W32.grad) < 1e-5 and rel(db, b32.grad) < 1e-5
    assert bool((dlast[:, 1:] == 0).all())  # every non-CLS row comes back exactly 0


for B in (37, 300):
    for kind, C in (("mse", 1), ("l1", 3), ("ce", 5), ("soft_ce", 10), ("soft_ce", 130), ("bce", 10), ("bce", 130)):
        add(f"vit_head_loss {kind} B={B} C={C}", ("vit_head_loss_fwd", "vit_head_loss_bwd"), functools.partial(head_loss, kind=kind, B=B, C=C))


# =================================================================================================== optimizer steps
OPT_N, OPT_CUT = 100_003, 50_000  # two parameter tensors / groups: [0, 50000) and [50000, 100003)
OPT_GROUPS = ((1e-3, 0.01, 0.9), (5e-4, 0.0, 0.5))  # (lr, weight_decay, momentum) per group


def opt_inputs(dev):
    gen = torch.Generator().manual_seed(1000 + OPT_N % 997)
    return torch.randn(OPT_N, generator=gen), torch.randn(OPT_N, generator=gen)


class bound_record:
    """A step record bound to the active handle for the block (the `_dyn` forms read their bias corrections from it);
    `advance()` restarts it and advances it to step 1, so every run of a case sees the same record."""

    def __init__(self, dev):
        from _poison import active_handle

        self.h, self.state = active_handle(dev), torch.zeros(8, dtype=torch.int32, device=dev)

    def __enter__(self):
        from vit_amd import _cabi

        _cabi.check(self.h.lib.vit_step_state_bind(self.h.h, self.state.data_ptr()), "vit_step_state_bind")
        return self

    def advance(self):
        import vit_amd.functional as vf
        from vit_amd import _cabi

        self.state.zero_()
        _cabi.check(self.h.lib.vit_step_advance(self.h.h, 0x1234567, 0.9, 0.999, vf._stream(self.state)), "vit_step_advance")

    def __exit__(self, *exc):
        from vit_amd import _cabi

        _cabi.check(self.h.lib.vit_step_state_bind(self.h.h, None), "vit_step_state_bind")
        return False


def opt_step(dev, kind, groups, dyn=False):
    """One step from a zero state against torch.optim on the CPU (tests/test_optim_gpu.py: rel < 1e-6, the shadow bf16(p)
    exactly).  p / m / v are in place: every run restarts them; the bf16 shadow is the pure output."""
    import vit_amd.functional as vf

    p0, g0 = opt_inputs(dev)
    parts = [slice(0, OPT_CUT), slice(OPT_CUT, OPT_N)] if groups else [slice(0, OPT_N)]
    twins = [p0[s].clone().requires_grad_(True) for s in parts]
    for tw, s in zip(twins, parts):
        tw.grad = g0[s].clone()
    hyper = OPT_GROUPS if groups else OPT_GROUPS[:1]
    if kind == "sgd":
        ref = torch.optim.SGD([dict(params=[tw], lr=lr, weight_decay=wd, momentum=mo) for tw, (lr, wd, mo) in zip(twins, hyper)], lr=1.0,
                              momentum=0.9, nesterov=True)  # the defaults only pass torch's nesterov check: every group sets its own
    else:
        cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
        ref = cls([dict(params=[tw], lr=lr, weight_decay=wd) for tw, (lr, wd, mo) in zip(twins, hyper)], lr=1.0)
    ref.step()
    want = torch.cat([tw.detach() for tw in twins])
    p0d, g = p0.to(dev), g0.to(dev)
    p, m, v, pb = E(dev, OPT_N), E(dev, OPT_N), E(dev, OPT_N), E(dev, OPT_N, dt=BF16)
    tables = None
    if groups:
        tables = vf.optim_group_tables([(0, OPT_CUT, 0), (OPT_CUT, OPT_N - OPT_CUT, 1)], 2, dev, total=OPT_N)
        vf.optim_groups_write(tables, hyper)
    lr, wd, mo = hyper[0]

    def run():
        p.copy_(p0d)
        m.zero_()
        v.zero_()
        if dyn:
            rec.advance()
        if kind == "sgd" and groups:
            vf.sgd_step_groups(p, g, m, pb, tables, nesterov=True, dyn=dyn)
        elif kind == "sgd":
            vf.sgd_step(p, g, m, pb, lr=lr, momentum=mo, weight_decay=wd, nesterov=True)
        elif groups:
            vf.adamw_step_groups(p, g, m, v, pb, tables, step=1, l2=kind == "adam_l2", dyn=dyn)
        else:
            (vf.adamw_step if kind == "adamw" else vf.adam_l2_step)(p, g, m, v, pb, lr=lr, weight_decay=wd, step=1)

    with bound_record(dev) if dyn else nothing() as rec:
        p, pb = poisoned(dev, run, [p, pb])
    assert rel(p.cpu(), want) < 1e-6, rel(p.cpu(), want)
    assert torch.equal(pb, bf(p))


for kind in ("adamw", "adam_l2", "sgd"):
    for groups in (False, True):
        add(f"vit_{kind}_step{'_groups' if groups else ''} n={OPT_N}", f"vit_{kind}_step{'_groups' if groups else ''}",
            functools.partial(opt_step, kind=kind, groups=groups))
    add(f"vit_{kind}_step_groups_dyn n={OPT_N} bound record at step 1", f"vit_{kind}_step_groups_dyn",
        functools.partial(opt_step, kind=kind, groups=True, dyn=True))


def lamb_step(dev, groups, dyn=False):
    """One LAMB step against the restatement of tests/_lamb_ref.py, within its own bound (4 x the f32 restatement's distance from
    the f64 one + 1 ulp, tests/test_lamb_gpu.py); the shadow is bf16(p) exactly.  Pure outputs: the shadow and `trust`."""
    import vit_amd.functional as vf
    from _lamb_ref import RefLamb, bound

    p0, g0 = opt_inputs(dev)
    g0 = g0 * 0.01
    parts = [slice(0, OPT_CUT), slice(OPT_CUT, OPT_N)] if groups else [slice(0, OPT_N)]
    hyper = ((1e-3, 0.05), (5e-4, 0.01)) if groups else ((1e-3, 0.05),)
    refs = {}
    for dt in (torch.float64, torch.float32):
        twins = [torch.nn.Parameter(p0[s].to(dt).clone()) for s in parts]
        for tw, s in zip(twins, parts):
            tw.grad = g0[s].to(dt).clone()
        opt = RefLamb([dict(params=[tw], lr=lr, weight_decay=wd) for tw, (lr, wd) in zip(twins, hyper)])
        opt.step()
        refs[dt] = [(tw.detach().clone(), opt.trust[id(tw)].clone()) for tw in twins]
    p0d, g = p0.to(dev), g0.to(dev)
    p, m, v, pb = E(dev, OPT_N), E(dev, OPT_N), E(dev, OPT_N), E(dev, OPT_N, dt=BF16)
    trust = E(dev, len(parts))
    if groups:
        tables = vf.optim_param_tables([(0, OPT_CUT, 0), (OPT_CUT, OPT_N - OPT_CUT, 1)], 2, dev, total=OPT_N)
        vf.optim_groups_write(tables, [(lr, wd, 0.0) for lr, wd in hyper])

    def run():
        p.copy_(p0d)
        m.zero_()
        v.zero_()
        if dyn:
            rec.advance()
        if groups:
            vf.lamb_step_groups(p, g, m, v, pb, tables, trust, step=1, dyn=dyn)
        else:
            vf.lamb_step(p, g, m, v, pb, lr=hyper[0][0], weight_decay=hyper[0][1], step=1, trust=trust)

    with bound_record(dev) if dyn else nothing() as rec:
        p, pb, trust = poisoned(dev, run, [p, pb, trust])
    assert torch.equal(pb, bf(p))
    for i, s in enumerate(parts):
        for got, j in ((p[s].cpu(), 0), (trust[i:i + 1].cpu(), 1)):
            r64, r32 = refs[torch.float64][i][j], refs[torch.float32][i][j]
            d32, allowed = bound(r64, r32)
            err = float((got.double().reshape(-1) - r64.double().reshape(-1)).abs().max())
            assert err <= allowed, (i, j, err, d32, allowed)
    if not groups:  # the by-value form without `trust`: the ratio lives in the workspace's 16-byte header
        p2, pb2 = E(dev, OPT_N), E(dev, OPT_N, dt=BF16)

        def run_no_trust():
            p2.copy_(p0d)
            m.zero_()
            v.zero_()
            vf.lamb_step(p2, g, m, v, pb2, lr=hyper[0][0], weight_decay=hyper[0][1], step=1)

        p2, pb2 = poisoned(dev, run_no_trust, [p2, pb2])
        assert torch.equal(p2, p) and torch.equal(pb2, pb)


add(f"vit_lamb_step n={OPT_N}", "vit_lamb_step", functools.partial(lamb_step, groups=False))
add(f"vit_lamb_step_groups n={OPT_N}", "vit_lamb_step_groups", functools.partial(lamb_step, groups=True))
add(f"vit_lamb_step_groups_dyn n={OPT_N} bound record at step 1", "vit_lamb_step_groups_dyn",
    functools.partial(lamb_step, groups=True, dyn=True))


# =================================================================================================== the remaining pure outputs
def ema_swap(dev):
    import vit_amd.functional as vf

    n = 1027
    gen = torch.Generator().manual_seed(1)
    p0, e0 = torch.randn(n, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev)
    p, ema, shadow = E(dev, n), E(dev, n), E(dev, n, dt=BF16)

    def run():
        p.copy_(p0)
        ema.copy_(e0)
        vf.ema_swap(p, ema, shadow)

    p, ema, shadow = poisoned(dev, run, [p, ema, shadow])
    assert torch.equal(p, e0) and torch.equal(ema, p0) and torch.equal(shadow, bf(e0))


add("vit_ema_swap n=1027 bf16 shadow", "vit_ema_swap", ema_swap)


def mix(dev, which):
    import vit_amd.functional as vf
    import _mix_ref as ref
    from test_mix_gpu import check_signal, check_targets, device_plan, plan_rows, target_rows

    if which == "signal":
        B, L = 5, 203
        x_host = torch.randn(B, L, generator=torch.Generator().manual_seed(100 + B + L))
        base = plan_rows(L)
        rows = [base[(1 + b) % len(base)] for b in range(B)]
        x, out, plan = x_host.to(dev), E(dev, B, L), device_plan(dev, rows)
        got, = poisoned(dev, lambda: vf.mix_signal(x, plan, B, out=out), [out])
        check_signal(x_host, got, rows, "poisoned mix_signal")
    elif which == "targets_reg":
        B, k = 5, 3
        y_host = torch.rand(B, k, generator=torch.Generator().manual_seed(20 + k))
        rows = target_rows(B)
        y, out, plan = y_host.to(dev), E(dev, B, k), device_plan(dev, rows)
        got, = poisoned(dev, lambda: vf.mix_targets(y, plan, B, out=out), [out])
        check_targets(got, *ref.mix_targets_reg(y_host.numpy(), rows), "poisoned mix_targets reg")
    else:
        B, C, s = 5, 7, 0.1
        y_host = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(30 + C))
        on, off = ref.on_off(s, C)
        rows = target_rows(B)
        y, out, plan = y_host.to(dev), E(dev, B, C), device_plan(dev, rows)
        got, = poisoned(dev, lambda: vf.mix_targets(y, plan, B, C, on, off, out=out), [out])
        check_targets(got, *ref.mix_targets_cls(y_host.numpy(), rows, C, s), "poisoned mix_targets cls")


add("vit_mix_signal (5, 203) copy form", "vit_mix_signal", functools.partial(mix, which="signal"))
add("vit_mix_targets regression (5, 3)", "vit_mix_targets", functools.partial(mix, which="targets_reg"))
add("vit_mix_targets classes (5, 7)", "vit_mix_targets", functools.partial(mix, which="targets_cls"))


def layer_scale_fold(dev, odt):
    import vit_amd.functional as vf

    g = torch.Generator().manual_seed(11)
    ents = []
    for rows, cols in ((5, 36), (64, 32)):
        lam = torch.exp(torch.empty(rows).uniform_(float(np.log(1e-6)), float(np.log(2.0)), generator=g))
        e = dict(W=torch.randn(rows, cols, generator=g).to(dev), b=torch.randn(rows, generator=g).to(dev), lam=lam.to(dev),
                 Wf=E(dev, rows, cols, dt=odt), bf=E(dev, rows))
        ents.append(e)
    tab = vf.layer_scale_table(ents, dev)
    outs = [e[k] for e in ents for k in ("Wf", "bf")]
    got = poisoned(dev, lambda: vf.layer_scale_fold(tab, odt), outs)
    for i, e in enumerate(ents):
        assert torch.equal(got[2 * i], (e["lam"][:, None] * e["W"]).to(odt)) and torch.equal(got[2 * i + 1], e["lam"] * e["b"])


for odt in (BF16, F32):
    add(f"vit_layer_scale_fold 5x36 + 64x32 {dn(odt)}", "vit_layer_scale_fold", functools.partial(layer_scale_fold, odt=odt))


def layer_scale_grad(dev):
    """Overwrite mode: dW, db, dlam are pure outputs; db_raw is zeroed in place, so every run restores it."""
    import vit_amd.functional as vf

    g = torch.Generator().manual_seed(23)
    ents, raw_b = [], []
    for rows, cols in ((5, 36), (64, 32)):
        lam = torch.exp(torch.empty(rows).uniform_(float(np.log(1e-6)), float(np.log(2.0)), generator=g))
        e = dict(W=torch.randn(rows, cols, generator=g).to(dev), b=torch.randn(rows, generator=g).to(dev), lam=lam.to(dev),
                 dW_raw=torch.randn(rows, cols, generator=g).to(dev), db_raw=E(dev, rows), dW=E(dev, rows, cols), db=E(dev, rows),
                 dlam=E(dev, rows))
        raw_b.append(torch.randn(rows, generator=g).to(dev))
        ents.append(e)
    tab = vf.layer_scale_table(ents, dev)

    def run():
        for e, rb in zip(ents, raw_b):
            e["db_raw"].copy_(rb)
        vf.layer_scale_grad(tab, False)

    got = poisoned(dev, run, [e[k] for e in ents for k in ("dW", "db", "dlam")])
    for i, (e, rb) in enumerate(zip(ents, raw_b)):
        dW, db, dlam = got[3 * i:3 * i + 3]
        assert torch.equal(dW, e["lam"][:, None] * e["dW_raw"]) and torch.equal(db, e["lam"] * rb)
        assert float(e["db_raw"].abs().max()) == 0.0
        terms = e["dW_raw"].double() * e["W"].double()  # tests/test_layerscale_gpu.py: the bound of any summation order
        exact = terms.sum(1) + rb.double() * e["b"].double()
        bound = (e["W"].shape[1] + 2) * 2.0 ** -24 * (terms.abs().sum(1) + (rb.double() * e["b"].double()).abs())
        assert bool(((dlam.double() - exact).abs() <= bound).all())


add("vit_layer_scale_grad 5x36 + 64x32 overwrite mode", "vit_layer_scale_grad", layer_scale_grad)


def add_noise(dev):
    """Only the distribution of the noise is contractual: level 0 is the identity bit for bit (tests/test_kernels_gpu.py); at
    level 0.5 the poison rounds alone judge (finite, the same bits over either fill)."""
    import vit_amd.functional as vf

    flux, err = randn((3, 1004), dev, 100), torch.rand((3, 1004), generator=torch.Generator().manual_seed(101)).to(dev) * 0.2 + 0.05
    out = E(dev, 3, 1004)
    got, = poisoned(dev, lambda: vf.add_noise(flux, err, 0.0, seed=1, out=out), [out])
    assert torch.equal(got, flux)
    got, = poisoned(dev, lambda: vf.add_noise(flux, err, 0.5, seed=1234, out=out), [out])
    assert not torch.equal(got, flux)


add("vit_add_noise (3, 1004)", "vit_add_noise", add_noise)


def patchdrop(dev, which):
    import vit_amd.functional as vf
    from _patchdrop_ref import positions, select, slot_of
    from test_patchdrop_gpu import random_idx

    B = 3
    if which == "select":
        B, N, K, seed, site = 5, 13, 3, 0x1234567, 49
        idx, slot = torch.empty((B, K), dtype=torch.int32, device=dev), torch.empty((B, N), dtype=torch.int32, device=dev)
        idx, slot = poisoned(dev, lambda: vf.patch_select(B, N, K, seed, site, idx, slot), [IntOut(idx, N - 1), IntOut(slot, K - 1)])
        e_idx, e_slot = select(B, N, K, seed, site)
        assert np.array_equal(idx.cpu().numpy(), e_idx) and np.array_equal(slot.cpu().numpy(), e_slot)
    elif which == "slot":
        N, K = 13, 3
        idx = random_idx(B, N, K, 305)
        slot = torch.empty((B, N), dtype=torch.int32, device=dev)
        slot, = poisoned(dev, lambda: vf.patch_slot(idx.to(dev), slot), [IntOut(slot, K - 1)])
        assert np.array_equal(slot.cpu().numpy(), slot_of(idx.numpy(), N))
    elif which == "unfold_gather":
        L, P, S, K = 103, 16, 12, 4
        N = -(-(L - P) // S) + 1
        x = randn((B, L), dev, 301)
        idx = random_idx(B, N, K, 302, must=N - 1).to(dev)  # the ragged last window is selected
        for odt in (BF16, F32):
            out = E(dev, B * K, P, dt=odt)
            got, = poisoned(dev, lambda: vf.unfold_gather_cast(x, idx, P, S, N, out=out), [out])
            full = x.unfold(1, P, S)
            full = torch.cat([full, torch.zeros(B, N - full.size(1), P, device=dev)], 1)
            assert torch.equal(got.view(B, K, P), torch.gather(full, 1, idx.long()[:, :, None].expand(B, K, P)).to(odt))
    elif which == "rows_gather":
        N, K, W = 40, 17, 8
        idx = random_idx(B, N, K, 341)
        table = randn((N + 1, W), dev, 343)
        out = E(dev, B * (K + 1), W)
        got, = poisoned(dev, lambda: vf.rows_gather(table, idx.to(dev), out=out), [out])
        assert torch.equal(got, table[torch.from_numpy(positions(idx.numpy())).to(dev)].view(B * (K + 1), W))
    elif which == "fold_add_gather":
        L, P, S, K = 103, 16, 12, 4
        N = -(-(L - P) // S) + 1
        idx = random_idx(B, N, K, 351, must=N - 1)
        slot = torch.from_numpy(slot_of(idx.numpy(), N)).to(dev)
        dp = randn((B * K, P), dev, 352)
        out = E(dev, B, L)
        got, = poisoned(dev, lambda: vf.fold_add_gather(dp, slot, L, P, S, out=out), [out])
        scattered = torch.zeros(B, N, P, dtype=torch.float64, device=dev)
        scattered[torch.arange(B, device=dev)[:, None].expand(B, K), idx.to(dev).long()] = dp.double().view(B, K, P)
        x = torch.zeros((B, L), dtype=torch.float64, device=dev, requires_grad=True)
        u = x.unfold(1, P, S)
        u = torch.cat([u, torch.zeros(B, N - u.size(1), P, dtype=torch.float64, device=dev)], 1)
        u.backward(scattered)
        assert rel(got, x.grad) < 1e-6 and float(got.abs().max()) > 0
    else:
        B, D, N, K, p, seed = 5, 32, 13, 5, 0.1, 41
        Tc = K + 1
        idx = random_idx(B, N - 1, K, 321)  # patch N - 1 is one that no sample kept
        slot = torch.from_numpy(slot_of(idx.numpy(), N)).to(dev)
        dtok = randn((B, Tc, D), dev, 323)
        g = dtok * drop_mult((p, seed, 0), B * Tc, D, dev).view(B, Tc, D)
        dpatch, dcls, dpos = E(dev, B * K, D, dt=BF16), E(dev, D), E(dev, N + 1, D)
        dpatch, dcls, dpos = poisoned(dev, lambda: vf.embed_finish_gather_bwd(dtok, slot, dcls, dpos, dropout=(p, seed, 0), dpatch=dpatch),
                                      [dpatch, dcls, dpos])
        assert torch.equal(dpatch.view(B, K, D), bf(g[:, 1:]))
        terms = torch.zeros(B, N + 1, D, dtype=torch.float64, device=dev)
        terms[:, 0] = g[:, 0].double()
        terms[torch.arange(B, device=dev)[:, None].expand(B, K), 1 + idx.to(dev).long()] = g[:, 1:].double()
        assert rel(dcls, terms[:, 0].sum(0)) < 1e-6 and rel(dpos, terms.sum(0)) < 1e-6
        assert bool((dpos[N] == 0).all())  # the row of the patch no sample kept is written, as zeros


add("vit_patch_select (5, 13, 3)", "vit_patch_select", functools.partial(patchdrop, which="select"))
add("vit_patch_slot (3, 13, 3)", "vit_patch_slot", functools.partial(patchdrop, which="slot"))
add("vit_unfold_gather_cast L=103 P=16 S=12 K=4", "vit_unfold_gather_cast", functools.partial(patchdrop, which="unfold_gather"))
add("vit_rows_gather (3, 17) of 41 rows", "vit_rows_gather", functools.partial(patchdrop, which="rows_gather"))
add("vit_fold_add_gather L=103 P=16 S=12 K=4", "vit_fold_add_gather", functools.partial(patchdrop, which="fold_add_gather"))
add("vit_embed_finish_gather_bwd (5, 6, 32)", "vit_embed_finish_gather_bwd", functools.partial(patchdrop, which="embed_bwd"))


def covariance(dev):
    """Mean and covariance of (300, 200) rows, two row slices in the workspace; tests/test_covstats_gpu.py's f32-chain bound."""
    import vit_amd.functional as vf
    from test_covstats_gpu import EPS as CEPS, case, worst_ratio

    n, L = 300, 200
    X, mean64, C64, bound = case(n, L, 100.0)
    x = X.to(dev)
    mean, acc, cov = E(dev, L), E(dev, L, L), E(dev, L, L)

    def run():
        vf.colsum(x, out=mean)
        vf.cov_mean_finish(mean, n)
        acc.zero_()  # accumulates by contract
        vf.cov_accumulate(x, mean, acc)
        vf.cov_finish(acc, n, out=cov)

    mean, cov = poisoned(dev, run, [mean, cov])
    assert float(((mean.cpu().double() - mean64).abs() / (n * CEPS * X.double().abs().mean(0))).max()) <= 1.0
    cov = cov.cpu()
    assert torch.equal(cov, cov.t()) and worst_ratio(cov, C64, bound) <= 1.0


add("vit_cov (300, 200): mean, accumulate over two slices, finish", ("vit_cov_mean_finish", "vit_cov_accumulate", "vit_cov_finish"), covariance)


# ===================================================================================================
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_poison(dev, case):
    case.fn(dev)
