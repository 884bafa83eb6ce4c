"""Tensor-level wrappers over the C ABI (include/vit_amd.h).  torch supplies device memory and the current HIP stream;
every computation happens in libvit_amd.so.  No function here has a PyTorch / CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _cabi
from ._cabi import ACT_DGELU, ACT_GELU, ACT_GELU_GRAD, ACT_MUL_AUX, ACT_NONE, LOSS_BCE, LOSS_CE, LOSS_L1, LOSS_MSE, LOSS_SOFT_CE, VIT_BF16, VIT_F32, GemmDesc

_DT = {torch.float32: VIT_F32, torch.bfloat16: VIT_BF16}


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


_HANDLE_OVERRIDE: Optional[_cabi.Handle] = None


def _h(t: torch.Tensor) -> _cabi.Handle:
    if not t.is_cuda:
        raise _cabi.VitError("vit_amd kernels need tensors on an MI355X (cuda/hip device); there is no CPU path")
    return _HANDLE_OVERRIDE if _HANDLE_OVERRIDE is not None else _cabi.handle_for(t.device)


class use_handle:
    """Route the calls inside the block through another vit_handle (its own workspace): what runs concurrently on a second
    HIP stream must not share split-K slabs / reduction partials with the main stream's kernels."""

    def __init__(self, handle: _cabi.Handle):
        self.handle = handle

    def __enter__(self):
        global _HANDLE_OVERRIDE
        self.prev, _HANDLE_OVERRIDE = _HANDLE_OVERRIDE, self.handle
        return self.handle

    def __exit__(self, *exc):
        global _HANDLE_OVERRIDE
        _HANDLE_OVERRIDE = self.prev
        return False


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype:
        raise _cabi.VitError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _cabi.VitError(f"{name}: tensor must be contiguous")


Dropout = Tuple[float, int, int]  # (p, seed, site)
NO_DROP: Dropout = (0.0, 0, 0)


# ------------------------------------------------------------------------------------------------ GEMM
def gemm(a: torch.Tensor, b: torch.Tensor, *, M: int, N: int, K: int, a_trans: bool = False, b_trans: bool = False,
         lda: Optional[int] = None, ldb: Optional[int] = None, out: Optional[torch.Tensor] = None,
         out_dtype=torch.bfloat16, ldc: Optional[int] = None, alpha: float = 1.0, bias: Optional[torch.Tensor] = None,
         act: int = ACT_NONE, aux_out: Optional[torch.Tensor] = None, aux_in: Optional[torch.Tensor] = None,
         dropout: Dropout = NO_DROP, residual: Optional[torch.Tensor] = None, row_map: Tuple[int, int, int] = (0, 0, 0),
         out_rows: Optional[int] = None, split_k: int = 0, accumulate: bool = False,
         colsum_out: Optional[torch.Tensor] = None,
         rope: Optional[Tuple[torch.Tensor, torch.Tensor, int, int, int]] = None, drop_row_stride: int = 0,
         ldaux: Optional[int] = None, ldres: Optional[int] = None) -> torch.Tensor:
    """`drop_row_stride = s > 1`: the dropout mask of output row r is the one of row r * s (the rows are a strided subset of
    a larger problem's: A read in place with `lda = s * K`, compact output).
    `rope = (cos, sin, T, head_dim, cols)`: rotary embedding of columns [0, cols) of the output (the q / k thirds of a fused QKV
    projection; cos / sin: f32 [T, head_dim / 2], rows = the reference's LINEAR zero-based positions t * theta_i -- the rotating
    epilogue steps angles by a recurrence over table row 8; other tables: `rope_qk`) -- in the GEMM's epilogue where the kernel can, by a vit_rope_qk pass behind it
    otherwise (the library decides; same result contract)."""
    h = _h(a)
    if a.dtype != b.dtype or a.dtype not in _DT:
        raise _cabi.VitError(f"gemm: operands must both be bf16 or both f32 (got {a.dtype}, {b.dtype})")
    if out is None:
        out = torch.empty((out_rows if out_rows is not None else M, N), dtype=out_dtype, device=a.device)
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.a_trans, d.b_trans = int(a_trans), int(b_trans)
    d.ab_dtype = _DT[a.dtype]  # f32 operands: split-bf16 "x3" kernel (fp32-class results)
    d.A, d.lda = a.data_ptr(), lda if lda is not None else (M if a_trans else K)
    d.B, d.ldb = b.data_ptr(), ldb if ldb is not None else (N if b_trans else K)
    d.C, d.ldc, d.c_dtype = out.data_ptr(), ldc if ldc is not None else N, _DT[out.dtype]
    d.alpha = alpha
    d.bias = _ptr(bias)
    d.act = act
    d.aux_out, d.aux_in, d.ldaux = _ptr(aux_out), _ptr(aux_in), ldaux if ldaux is not None else N
    d.dropout_p, d.seed, d.site = dropout
    d.drop_row_stride = int(drop_row_stride)
    d.residual, d.ldres = _ptr(residual), ldres if ldres is not None else N
    d.rows_per_batch, d.out_batch_rows, d.out_row_offset = row_map
    d.split_k = split_k
    d.accumulate = int(accumulate)
    if colsum_out is not None:  # column sums of C (a bias gradient): fused into the epilogue or a vit_colsum pass
        _chk(colsum_out, torch.float32, "gemm colsum_out")
        if colsum_out.numel() != N:
            raise _cabi.VitError(f"gemm: colsum_out must have N={N} elements")
        d.colsum_out = colsum_out.data_ptr()
    if rope is not None:
        cos, sin, rT, rdh, rcols = rope
        _chk(cos, torch.float32, "gemm rope cos")
        _chk(sin, torch.float32, "gemm rope sin")
        if cos.numel() != rT * (rdh // 2) or sin.numel() != cos.numel():
            raise _cabi.VitError(f"gemm: rope tables must be [T={rT}, head_dim/2={rdh // 2}]")
        d.rope_cos, d.rope_sin, d.rope_T, d.rope_dh, d.rope_cols = cos.data_ptr(), sin.data_ptr(), int(rT), int(rdh), int(rcols)
    h.call("vit_gemm", C.byref(d), _stream(a))
    return out


def linear_fwd(x, W, bias=None, *, out_dtype=torch.bfloat16, act=ACT_NONE, aux_out=None, dropout: Dropout = NO_DROP,
               residual=None, out=None):
    M, K = x.shape
    N = W.shape[0]
    return gemm(x, W, M=M, N=N, K=K, out=out, out_dtype=out_dtype, bias=bias, act=act, aux_out=aux_out, dropout=dropout,
                residual=residual)


def linear_bwd_dx(dy, W, *, out_dtype=torch.bfloat16, dgelu_aux=None, out=None):
    M, N = dy.shape
    K = W.shape[1]
    return gemm(dy, W, M=M, N=K, K=N, b_trans=True, out=out, out_dtype=out_dtype,
                act=ACT_DGELU if dgelu_aux is not None else ACT_NONE, aux_in=dgelu_aux)


def linear_bwd_dw(dy, x, *, out=None, accumulate=False):
    M, N = dy.shape
    K = x.shape[1]
    return gemm(dy, x, M=N, N=K, K=M, a_trans=True, b_trans=True, out=out, out_dtype=torch.float32, split_k=-1,
                accumulate=accumulate)


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, gamma, beta, eps: float, out_dtype=torch.bfloat16, out=None, mean=None, rstd=None):
    _chk(x, torch.float32, "layernorm_fwd x")
    h = _h(x)
    D = x.shape[-1]
    rows = x.numel() // D
    y = out if out is not None else torch.empty(x.shape, dtype=out_dtype, device=x.device)
    mean = mean if mean is not None else torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = rstd if rstd is not None else torch.empty(rows, dtype=torch.float32, device=x.device)
    h.call("vit_layernorm_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _DT[y.dtype], _ptr(mean),
           _ptr(rstd), rows, D, eps, _stream(x))
    return y, mean, rstd


DropPath = Tuple[float, int, int, int]  # (p, site, rows_per_sample, branch); the seed is the step's, shared with dropout


def layernorm_fwd_residual(x, delta, xsum, gamma, beta, eps: float, out_dtype=torch.bfloat16, out=None, mean=None,
                           rstd=None, x_row_stride: int = 1, path: Optional[DropPath] = None, seed: int = 0):
    """xsum = x + delta (f32 stream + bf16/f32 projection output); y = LayerNorm(xsum).
    `x_row_stride = s > 1`: the rows are every s-th row of x (delta, xsum, y, mean, rstd compact: x.numel() / (D s) rows).
    `path` (with `seed`): the stochastic-depth form, see layernorm_fwd_residual_path."""
    _chk(x, torch.float32, "layernorm_fwd_residual x")
    _chk(xsum, torch.float32, "layernorm_fwd_residual xsum")
    h = _h(x)
    D = x.shape[-1]
    rows = xsum.numel() // D
    if x_row_stride < 1 or (rows - 1) * x_row_stride * D + D > x.numel() or (x_row_stride == 1 and x.numel() != xsum.numel()):
        raise _cabi.VitError("layernorm_fwd_residual: x does not hold the rows that xsum and x_row_stride name")
    if delta.dtype not in _DT or not delta.is_contiguous() or delta.numel() != xsum.numel():
        raise _cabi.VitError("layernorm_fwd_residual: delta must be a contiguous bf16/f32 tensor of xsum's shape")
    y = out if out is not None else torch.empty(xsum.shape, dtype=out_dtype, device=x.device)
    mean = mean if mean is not None else torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = rstd if rstd is not None else torch.empty(rows, dtype=torch.float32, device=x.device)
    if y.numel() != xsum.numel() or mean.numel() < rows or rstd.numel() < rows:
        raise _cabi.VitError("layernorm_fwd_residual: out / mean / rstd do not hold xsum's rows")
    if path is not None:
        p, site, rps, branch = path
        h.call("vit_layernorm_fwd_residual_path", x.data_ptr(), x_row_stride, delta.data_ptr(), _DT[delta.dtype],
               xsum.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _DT[y.dtype], _ptr(mean), _ptr(rstd), rows,
               D, eps, p, seed, site, rps, branch, _stream(x))
        return y, mean, rstd
    if x_row_stride != 1:
        h.call("vit_layernorm_fwd_residual_rows", x.data_ptr(), x_row_stride, delta.data_ptr(), _DT[delta.dtype],
               xsum.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _DT[y.dtype], _ptr(mean), _ptr(rstd), rows,
               D, eps, _stream(x))
        return y, mean, rstd
    h.call("vit_layernorm_fwd_residual", x.data_ptr(), delta.data_ptr(), _DT[delta.dtype], xsum.data_ptr(),
           gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _DT[y.dtype], _ptr(mean), _ptr(rstd), rows, D, eps, _stream(x))
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dres=None, dx=None, dgamma=None, dbeta=None):
    _chk(x, torch.float32, "layernorm_bwd x")
    h = _h(x)
    D = x.shape[-1]
    rows = x.numel() // D
    dx = dx if dx is not None else torch.empty_like(x)
    dgamma = dgamma if dgamma is not None else torch.empty(D, dtype=torch.float32, device=x.device)
    dbeta = dbeta if dbeta is not None else torch.empty(D, dtype=torch.float32, device=x.device)
    h.call("vit_layernorm_bwd", dy.data_ptr(), _DT[dy.dtype], x.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
           rstd.data_ptr(), _ptr(dres), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), rows, D, _stream(x))
    return dx, dgamma, dbeta


def layernorm_bwd_fused(dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, dyn, dbias, dropout: Dropout = NO_DROP):
    """LayerNorm backward that also emits dyn = mask * dx (bf16) and dbias = colsum(dyn)."""
    _chk(x, torch.float32, "layernorm_bwd_fused x")
    h = _h(x)
    D = x.shape[-1]
    rows = x.numel() // D
    p, seed, site = dropout
    h.call("vit_layernorm_bwd_fused", dy.data_ptr(), _DT[dy.dtype], x.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
           rstd.data_ptr(), _ptr(dres), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), rows, D, dyn.data_ptr(),
           _DT[dyn.dtype], dbias.data_ptr(), p, seed, site, _stream(x))
    return dx, dgamma, dbeta, dyn, dbias


def layernorm_bwd_rows(dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, dyn=None, dbias=None, dropout: Dropout = NO_DROP,
                       dres_row_stride: int = 0, row_stride: int = 1, full_rows: Optional[int] = None,
                       path: Optional[DropPath] = None):
    """layernorm_bwd (dyn None) / layernorm_bwd_fused at the two ends of a compact run of rows (vit_layernorm_bwd_rows):
    `row_stride = s > 1`: the tensors hold the rows r = j * s of a full tensor of `full_rows` rows compactly (mask keyed by r,
    parameter gradients summed in the full pass's order); `dres_row_stride = s > 0`: dres alone is compact and its row j is the
    residual gradient of row j * s, every other row has none.  `path` (with dyn): the stochastic-depth form, see
    layernorm_bwd_path."""
    _chk(x, torch.float32, "layernorm_bwd_rows x")
    _chk(dx, torch.float32, "layernorm_bwd_rows dx")
    h = _h(x)
    D = x.shape[-1]
    rows = x.numel() // D
    if dy.numel() != x.numel() or dx.numel() != x.numel() or mean.numel() < rows or rstd.numel() < rows or \
            (dyn is not None and (dyn.numel() != x.numel() or dbias is None)):
        raise _cabi.VitError("layernorm_bwd_rows: dy / dx / dyn must have x's shape, mean / rstd its rows")
    if dres is not None:
        _chk(dres, torch.float32, "layernorm_bwd_rows dres")
        need = x.numel() if dres_row_stride == 0 else -(-rows // dres_row_stride) * D
        if dres_row_stride < 0 or dres.numel() < need:
            raise _cabi.VitError(f"layernorm_bwd_rows: dres holds {dres.numel()} elements, needs {need}")
    p, seed, site = dropout
    if row_stride > 1:
        full_rows = (rows - 1) * row_stride + 1 if full_rows is None else full_rows
        if dres_row_stride or -(-full_rows // row_stride) != rows:
            raise _cabi.VitError("layernorm_bwd_rows: row_stride needs full_rows = the full tensor's rows and a dres like dx")
        rows = full_rows
    if path is not None:
        pp, psite, rps, branch = path
        h.call("vit_layernorm_bwd_path", dy.data_ptr(), _DT[dy.dtype], x.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
               rstd.data_ptr(), _ptr(dres), dres_row_stride, dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), rows, D,
               _ptr(dyn), _DT[dyn.dtype] if dyn is not None else VIT_BF16, _ptr(dbias), p, seed, site, row_stride, pp, psite,
               rps, branch, _stream(x))
        return dx
    h.call("vit_layernorm_bwd_rows", dy.data_ptr(), _DT[dy.dtype], x.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
           rstd.data_ptr(), _ptr(dres), dres_row_stride, dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), rows, D,
           _ptr(dyn), _DT[dyn.dtype] if dyn is not None else VIT_BF16, _ptr(dbias), p, seed, site, row_stride, _stream(x))
    return dx


def layernorm_fwd_residual_path(x, delta, xsum, gamma, beta, eps: float, path: DropPath, seed: int, **kw):
    """layernorm_fwd_residual with a per-sample gate on delta (include/vit_amd_droppath.h): xsum = x + m * delta, m = 0 or the
    kept-branch scale, one draw per (sample, branch); the sample of compact row r is r * x_row_stride // rows_per_sample."""
    return layernorm_fwd_residual(x, delta, xsum, gamma, beta, eps, path=path, seed=seed, **kw)


def layernorm_bwd_path(dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, dyn, dbias, path: DropPath, **kw):
    """layernorm_bwd_rows (its fused form: dyn and dbias are required) for a sum whose branch is gated per sample
    (include/vit_amd_droppath.h): dyn = dx * dropout mask * (0 or the kept-branch scale); the seed is `dropout`'s, also with
    dropout off; the sample of full row r is r // rows_per_sample."""
    if dyn is None or dbias is None:
        raise _cabi.VitError("layernorm_bwd_path: dyn and dbias are required")
    return layernorm_bwd_rows(dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, dyn=dyn, dbias=dbias, path=path, **kw)


def linear_bwd_dw_rows(dy, x, out, *, row_stride: int, full_rows: int, ldx: Optional[int] = None):
    """out[N, K] (f32) = dy^T x over compact rows that stand for the rows b * row_stride of full tensors of `full_rows` rows,
    summed in the full product's order where that product would run the ping-pong core (vit_linear_bwd_dw_rows)."""
    _chk(out, torch.float32, "linear_bwd_dw_rows out")
    if dy.dtype != x.dtype or dy.dtype not in _DT:
        raise _cabi.VitError("linear_bwd_dw_rows: operands must both be bf16 or both f32")
    h = _h(dy)
    rows, N = dy.shape
    K = out.shape[1]
    if out.shape[0] != N or not out.is_contiguous() or not dy.is_contiguous():
        raise _cabi.VitError("linear_bwd_dw_rows: out must be a contiguous [N, K] tensor, dy contiguous")
    h.call("vit_linear_bwd_dw_rows", dy.data_ptr(), N, x.data_ptr(), ldx if ldx is not None else K, _DT[dy.dtype],
           out.data_ptr(), rows, N, K, row_stride, full_rows, _stream(dy))
    return out


def colsum_rows(a, out, *, row_stride: int, full_rows: int):
    """out[cols] = column sums of compact a, in the order of the fused column sums over the full tensor (vit_colsum_rows)."""
    _chk(out, torch.float32, "colsum_rows out")
    h = _h(a)
    rows, cols = a.shape
    h.call("vit_colsum_rows", a.data_ptr(), _DT[a.dtype], a.stride(0), out.data_ptr(), rows, cols, row_stride, full_rows,
           _stream(a))
    return out


# ------------------------------------------------------------------------------------------------ attention
def attention_fwd(qkv, B: int, H: int, T: int, dh: int, scale: float, dropout: Dropout = NO_DROP, ctx=None, lse=None,
                  ctx_lo=None):
    """ctx_lo (bf16, like ctx): also store the rounding residual of the context for the backward's delta (vit_amd.h)."""
    h = _h(qkv)
    ctx = ctx if ctx is not None else torch.empty((B * T, H * dh), dtype=qkv.dtype, device=qkv.device)
    lse = lse if lse is not None else torch.empty((B * H, T), dtype=torch.float32, device=qkv.device)
    p, seed, site = dropout
    if ctx_lo is not None:
        _chk(ctx_lo, ctx.dtype, "attention_fwd ctx_lo")
    h.call("vit_attention_fwd", qkv.data_ptr(), ctx.data_ptr(), _ptr(ctx_lo), lse.data_ptr(), _DT[qkv.dtype], B, H, T, dh,
           scale, p, seed, site, _stream(qkv))
    return ctx, lse


def attention_bwd(qkv, ctx, dctx, lse, B: int, H: int, T: int, dh: int, scale: float, dropout: Dropout = NO_DROP,
                  dqkv=None, delta=None, colsum_out=None, ctx_lo=None):
    """colsum_out (f32 [3*H*dh]): also the column sums of dqkv (the QKV projection's bias gradient).
    ctx_lo: the residual attention_fwd(ctx_lo=...) stored."""
    _chk(dctx, qkv.dtype, "attention_bwd dctx")
    h = _h(qkv)
    dqkv = dqkv if dqkv is not None else torch.empty_like(qkv)
    delta = delta if delta is not None else torch.empty((B * H, T), dtype=torch.float32, device=qkv.device)
    p, seed, site = dropout
    if colsum_out is not None:
        _chk(colsum_out, torch.float32, "attention_bwd colsum_out")
    h.call("vit_attention_bwd", qkv.data_ptr(), ctx.data_ptr(), _ptr(ctx_lo), dctx.data_ptr(), lse.data_ptr(),
           delta.data_ptr(), dqkv.data_ptr(), _DT[qkv.dtype], B, H, T, dh, scale, p, seed, site, _ptr(colsum_out),
           _stream(qkv))
    return dqkv


def attention_probs(qkv, B: int, H: int, T: int, dh: int, scale: float, out=None):
    h = _h(qkv)
    probs = out if out is not None else torch.empty((B, H, T, T), dtype=torch.float32, device=qkv.device)
    _chk(probs, torch.float32, "attention_probs out")
    if probs.numel() != B * H * T * T:
        raise _cabi.VitError("attention_probs: out must hold [B, H, T, T]")
    h.call("vit_attention_probs", qkv.data_ptr(), probs.data_ptr(), _DT[qkv.dtype], B, H, T, dh, scale, _stream(qkv))
    return probs


# ------------------------------------------------------------------------------------------------ embedding side
def fold_add(dpatches, B: int, L: int, P: int, S: int, N: int, out=None):
    """dx[B, L] = overlap-add of dpatches [B*N, P] (f32): the backward of unfold_cast wrt the signal."""
    _chk(dpatches, torch.float32, "fold_add dpatches")
    if dpatches.numel() != B * N * P:
        raise _cabi.VitError("fold_add: dpatches must hold B*N*P elements")
    out = out if out is not None else torch.empty((B, L), dtype=torch.float32, device=dpatches.device)
    h = _h(dpatches)
    h.call("vit_fold_add", dpatches.data_ptr(), out.data_ptr(), B, L, P, S, N, _stream(dpatches))
    return out


def add_noise(flux, error, noise_level: float, seed: int, out=None):
    """flux + N(0,1) * error * noise_level (vit.py:86-88), counter-based normals keyed on (seed, element index)."""
    _chk(flux, torch.float32, "add_noise flux")
    _chk(error, torch.float32, "add_noise error")
    if error.shape != flux.shape or flux.numel() % 4:
        raise _cabi.VitError("add_noise: flux/error must have the same shape and a multiple of 4 elements")
    out = out if out is not None else torch.empty_like(flux)
    h = _h(flux)
    h.call("vit_add_noise", flux.data_ptr(), error.data_ptr(), out.data_ptr(), flux.numel(), float(noise_level),
           int(seed) & 0xFFFFFFFFFFFFFFFF, _stream(flux))
    return out


def rope_qk(qkv, cos_half, sin_half, T: int, H: int, dh: int, inverse: bool = False):
    """In-place rotary embedding of the q and k thirds of qkv [B*T, 3*H*dh] (bf16 or f32); cos/sin f32 [>=T, dh/2]."""
    if qkv.dtype not in _DT or not qkv.is_contiguous() or qkv.dim() != 2 or qkv.shape[1] != 3 * H * dh:
        raise _cabi.VitError(f"rope_qk: qkv must be a contiguous [rows, {3 * H * dh}] bf16/f32 tensor")
    _chk(cos_half, torch.float32, "rope_qk cos")
    _chk(sin_half, torch.float32, "rope_qk sin")
    if cos_half.shape[-1] != dh // 2 or cos_half.shape[0] < T or sin_half.shape != cos_half.shape:
        raise _cabi.VitError("rope_qk: tables must be [>= T, dh/2]")
    h = _h(qkv)
    h.call("vit_rope_qk", qkv.data_ptr(), _DT[qkv.dtype], cos_half.data_ptr(), sin_half.data_ptr(), qkv.shape[0], T, H, dh,
           qkv.shape[1], 1 if inverse else 0, _stream(qkv))
    return qkv


def unfold_cast(x, P: int, S: int, N: int, out=None, out_dtype=torch.bfloat16):
    _chk(x, torch.float32, "unfold_cast x")
    h = _h(x)
    B, L = x.shape
    out = out if out is not None else torch.empty((B * N, P), dtype=out_dtype, device=x.device)
    h.call("vit_unfold_cast", x.data_ptr(), out.data_ptr(), _DT[out.dtype], B, L, P, S, N, _stream(x))
    return out


def embed_finish(tokens, cls, pos=None, dropout: Dropout = NO_DROP):
    _chk(tokens, torch.float32, "embed_finish tokens")
    h = _h(tokens)
    B, T, D = tokens.shape
    p, seed, site = dropout
    h.call("vit_embed_finish", tokens.data_ptr(), cls.data_ptr(), _ptr(pos), B, T, D, p, seed, site, _stream(tokens))
    return tokens


def embed_finish_bwd(dtokens, dcls, dpos=None, dropout: Dropout = NO_DROP, dpatch=None, out_dtype=torch.bfloat16):
    _chk(dtokens, torch.float32, "embed_finish_bwd dtokens")
    h = _h(dtokens)
    B, T, D = dtokens.shape
    dpatch = dpatch if dpatch is not None else torch.empty((B * (T - 1), D), dtype=out_dtype, device=dtokens.device)
    p, seed, site = dropout
    h.call("vit_embed_finish_bwd", dtokens.data_ptr(), dpatch.data_ptr(), _DT[dpatch.dtype], dcls.data_ptr(), _ptr(dpos), B,
           T, D, p, seed, site, 0, _stream(dtokens))
    return dpatch


# ------------------------------------------------------------------------------------------------ patch dropout
def _chk_index(t: torch.Tensor, B: int, cols: int, name: str):
    _chk(t, torch.int32, name)
    if not t.is_cuda or tuple(t.shape) != (B, cols):
        raise _cabi.VitError(f"{name}: expected an int32 [{B}, {cols}] device tensor, got {tuple(t.shape)} on {t.device}")


def patch_select(B: int, N: int, K: int, seed: int, site: int, idx, slot):
    """The per-sample K-subset of N patches drawn from (seed, site) (vit_patch_select): idx int32 [B, K] ascending, slot int32
    [B, N] its inverse (-1: dropped).  A step record bound to the handle varies the draw per replay."""
    _chk_index(idx, B, K, "patch_select idx")
    _chk_index(slot, B, N, "patch_select slot")
    _h(idx).call("vit_patch_select", idx.data_ptr(), slot.data_ptr(), B, N, K, int(seed) & 0xFFFFFFFFFFFFFFFF, int(site),
                 _stream(idx))
    return idx, slot


def patch_slot(idx, slot):
    """slot [B, N] <- the inverse map of a given idx [B, K] (vit_patch_slot)."""
    B, N = slot.shape
    _chk_index(slot, B, N, "patch_slot slot")
    _chk_index(idx, B, idx.shape[1], "patch_slot idx")
    _h(idx).call("vit_patch_slot", idx.data_ptr(), slot.data_ptr(), B, N, idx.shape[1], _stream(idx))
    return slot


def unfold_gather_cast(x, idx, P: int, S: int, N: int, out=None, out_dtype=torch.bfloat16):
    """Rows b * N + idx[b, k] of unfold_cast's output, compact: [B * K, P]."""
    _chk(x, torch.float32, "unfold_gather_cast x")
    B, L = x.shape
    K = idx.shape[1]
    _chk_index(idx, B, K, "unfold_gather_cast idx")
    out = out if out is not None else torch.empty((B * K, P), dtype=out_dtype, device=x.device)
    if out.numel() != B * K * P or not out.is_contiguous():
        raise _cabi.VitError("unfold_gather_cast: out must be a contiguous [B*K, P] tensor")
    _h(x).call("vit_unfold_gather_cast", x.data_ptr(), idx.data_ptr(), out.data_ptr(), _DT[out.dtype], B, L, P, S, N, K, _stream(x))
    return out


def embed_finish_gather(tokens, cls, idx, T_full: int, pos=None, dropout: Dropout = NO_DROP):
    """embed_finish over compact tokens [B, 1 + K, D]: token t > 0 takes position row 1 + idx[b, t - 1] of pos [T_full, D]; the
    mask is keyed by the compact row."""
    _chk(tokens, torch.float32, "embed_finish_gather tokens")
    B, Tc, D = tokens.shape
    _chk_index(idx, B, Tc - 1, "embed_finish_gather idx")
    if pos is not None and pos.numel() != T_full * D:
        raise _cabi.VitError(f"embed_finish_gather: pos must hold [T_full={T_full}, {D}]")
    p, seed, site = dropout
    _h(tokens).call("vit_embed_finish_gather", tokens.data_ptr(), cls.data_ptr(), _ptr(pos), idx.data_ptr(), B, Tc, T_full, D, p,
                    seed, site, _stream(tokens))
    return tokens


def embed_finish_gather_bwd(dtokens, slot, dcls, dpos=None, dropout: Dropout = NO_DROP, dpatch=None, out_dtype=torch.bfloat16,
                            accumulate: bool = False):
    """The backward of embed_finish_gather: dpatch [B * K, D]; dcls; dpos [T_full, D] summed through slot [B, T_full - 1]."""
    _chk(dtokens, torch.float32, "embed_finish_gather_bwd dtokens")
    B, Tc, D = dtokens.shape
    N = slot.shape[1]
    _chk_index(slot, B, N, "embed_finish_gather_bwd slot")
    if dpos is not None and dpos.numel() != (N + 1) * D:
        raise _cabi.VitError(f"embed_finish_gather_bwd: dpos must hold [{N + 1}, {D}]")
    dpatch = dpatch if dpatch is not None else torch.empty((B * (Tc - 1), D), dtype=out_dtype, device=dtokens.device)
    if dpatch.numel() != B * (Tc - 1) * D:
        raise _cabi.VitError("embed_finish_gather_bwd: dpatch must hold [B*K, D]")
    p, seed, site = dropout
    _h(dtokens).call("vit_embed_finish_gather_bwd", dtokens.data_ptr(), slot.data_ptr(), dpatch.data_ptr(), _DT[dpatch.dtype],
                     dcls.data_ptr(), _ptr(dpos), B, Tc, N + 1, D, p, seed, site, int(accumulate), _stream(dtokens))
    return dpatch


def rows_gather(table, idx, out=None):
    """out[b * Tc + t, :] = table[pos(b, t), :] (pos = 0 for t = 0, 1 + idx[b, t - 1] otherwise); table f32 [T_full, W]."""
    _chk(table, torch.float32, "rows_gather table")
    if table.dim() != 2:
        raise _cabi.VitError("rows_gather: table must be [T_full, W]")
    T_full, W = table.shape
    B, K = idx.shape
    _chk_index(idx, B, K, "rows_gather idx")
    out = out if out is not None else torch.empty((B * (K + 1), W), dtype=torch.float32, device=table.device)
    _chk(out, torch.float32, "rows_gather out")
    if out.numel() != B * (K + 1) * W:
        raise _cabi.VitError("rows_gather: out must hold [B*(K+1), W]")
    _h(table).call("vit_rows_gather", table.data_ptr(), idx.data_ptr(), out.data_ptr(), B, K + 1, T_full, W, _stream(table))
    return out


def fold_add_gather(dpatches, slot, L: int, P: int, S: int, out=None):
    """fold_add of compact dpatches [B * K, P] read through slot [B, N]: dropped windows contribute nothing."""
    _chk(dpatches, torch.float32, "fold_add_gather dpatches")
    B, N = slot.shape
    _chk_index(slot, B, N, "fold_add_gather slot")
    K = dpatches.numel() // (B * P)
    if dpatches.numel() != B * K * P or not 0 < K <= N:
        raise _cabi.VitError("fold_add_gather: dpatches must hold B*K*P elements with 1 <= K <= N")
    out = out if out is not None else torch.empty((B, L), dtype=torch.float32, device=dpatches.device)
    _h(dpatches).call("vit_fold_add_gather", dpatches.data_ptr(), slot.data_ptr(), out.data_ptr(), B, L, P, S, N, K,
                      _stream(dpatches))
    return out


# ------------------------------------------------------------------------------------------------ masked spectrum modelling
def mim_mask(slot_blocks, span: int, mask):
    """mask int32 [B, N] <- slot_blocks[b, n // span] < 0: the block selection [B, ceil(N / span)] expanded to patches."""
    B, N = mask.shape
    _chk_index(mask, B, N, "mim_mask mask")
    _chk_index(slot_blocks, B, slot_blocks.shape[1], "mim_mask slot_blocks")
    _h(mask).call("vit_mim_mask", slot_blocks.data_ptr(), mask.data_ptr(), B, N, slot_blocks.shape[1], int(span), _stream(mask))
    return mask


def embed_finish_masked(tokens, cls, mask, mask_token, pos=None, dropout: Dropout = NO_DROP):
    """embed_finish with the projected token of every masked patch (mask int32 [B, T - 1] non-zero) replaced by mask_token [D]."""
    _chk(tokens, torch.float32, "embed_finish_masked tokens")
    B, T, D = tokens.shape
    _chk_index(mask, B, T - 1, "embed_finish_masked mask")
    _chk(mask_token, torch.float32, "embed_finish_masked mask_token")
    if mask_token.numel() != D or cls.numel() != D or (pos is not None and pos.numel() != T * D):
        raise _cabi.VitError(f"embed_finish_masked: cls and mask_token must hold [{D}], pos [{T}, {D}]")
    p, seed, site = dropout
    _h(tokens).call("vit_embed_finish_masked", tokens.data_ptr(), cls.data_ptr(), _ptr(pos), mask.data_ptr(), mask_token.data_ptr(),
                    B, T, D, p, seed, site, _stream(tokens))
    return tokens


def embed_finish_masked_bwd(dtokens, mask, dcls, dmask_token, dpos=None, dropout: Dropout = NO_DROP, dpatch=None,
                            out_dtype=torch.bfloat16, accumulate: bool = False):
    """The backward of embed_finish_masked: dpatch [B * N, D] with exact zeros in the masked rows; dcls, dpos as
    embed_finish_bwd's; dmask_token [D] the sum over the masked rows."""
    _chk(dtokens, torch.float32, "embed_finish_masked_bwd dtokens")
    B, T, D = dtokens.shape
    _chk_index(mask, B, T - 1, "embed_finish_masked_bwd mask")
    _chk(dmask_token, torch.float32, "embed_finish_masked_bwd dmask_token")
    if dmask_token.numel() != D or dcls.numel() != D or (dpos is not None and dpos.numel() != T * D):
        raise _cabi.VitError(f"embed_finish_masked_bwd: dcls and dmask_token must hold [{D}], dpos [{T}, {D}]")
    dpatch = dpatch if dpatch is not None else torch.empty((B * (T - 1), D), dtype=out_dtype, device=dtokens.device)
    if dpatch.numel() != B * (T - 1) * D:
        raise _cabi.VitError("embed_finish_masked_bwd: dpatch must hold [B*N, D]")
    p, seed, site = dropout
    _h(dtokens).call("vit_embed_finish_masked_bwd", dtokens.data_ptr(), mask.data_ptr(), dpatch.data_ptr(), _DT[dpatch.dtype],
                     dcls.data_ptr(), _ptr(dpos), dmask_token.data_ptr(), B, T, D, p, seed, site, int(accumulate), _stream(dtokens))
    return dpatch


# ------------------------------------------------------------------------------------------------ register tokens
def _chk_reg(tokens, R: int, cls, reg, pos, mask, mask_token, who: str, mt_name: str):
    """The shape and dtype checks the two register entry points share; returns (B, N, D)."""
    _chk(tokens, torch.float32, who + " tokens")
    if isinstance(R, bool) or not isinstance(R, int) or R < 0:
        raise _cabi.VitError(f"{who}: R must be an integer >= 0, got {R!r}")
    if tokens.dim() != 3 or tokens.shape[1] < 2 + R:
        raise _cabi.VitError(f"{who}: tokens must be [B, 1 + R + N, D] with N >= 1, got {tuple(tokens.shape)} at R={R}")
    B, T, D = tokens.shape
    N = T - 1 - R
    _chk(cls, torch.float32, who + " cls")
    if R > 0:
        if reg is None:
            raise _cabi.VitError(f"{who}: R={R} needs the register tensor [{R}, {D}]")
        _chk(reg, torch.float32, who + " reg")
    if (mask is None) != (mask_token is None):
        raise _cabi.VitError(f"{who}: mask and {mt_name} go together")
    if mask is not None:
        _chk_index(mask, B, N, who + " mask")
        _chk(mask_token, torch.float32, f"{who} {mt_name}")
    if pos is not None:
        _chk(pos, torch.float32, who + " pos")
    if cls.numel() != D or (R > 0 and reg.numel() != R * D) or (mask_token is not None and mask_token.numel() != D) or \
            (pos is not None and pos.numel() != (1 + N) * D):
        raise _cabi.VitError(f"{who}: cls and {mt_name} must hold [{D}], reg [{R}, {D}], pos [{1 + N}, {D}]")
    return B, N, D


def embed_finish_reg(tokens, R: int, cls, reg, pos=None, mask=None, mask_token=None, dropout: Dropout = NO_DROP):
    """embed_finish / embed_finish_masked over tokens [B, 1 + R + N, D] with R register rows behind CLS (vit_embed_finish_reg):
    row 0 <- cls, rows 1 .. R <- reg [R, D], a masked patch (mask int32 [B, N] non-zero) <- mask_token; pos [1 + N, D] is added to
    CLS (row 0) and patch n (row 1 + n), nothing to a register; dropout over every row.  In place."""
    B, N, D = _chk_reg(tokens, R, cls, reg, pos, mask, mask_token, "embed_finish_reg", "mask_token")
    p, seed, site = dropout
    _h(tokens).call("vit_embed_finish_reg", tokens.data_ptr(), cls.data_ptr(), _ptr(reg if R > 0 else None), _ptr(pos), _ptr(mask),
                    _ptr(mask_token), B, R, N, D, p, seed, site, _stream(tokens))
    return tokens


def embed_finish_reg_bwd(dtokens, R: int, dcls, dreg, dpos=None, mask=None, dmask_token=None, dropout: Dropout = NO_DROP,
                         dpatch=None, out_dtype=torch.bfloat16, accumulate: bool = False):
    """The backward of embed_finish_reg: dpatch [B * N, D] (exact zeros in masked rows); dcls [D], dreg [R, D], dpos [1 + N, D],
    dmask_token [D] (with a mask) as batch sums in the order of include/vit_amd_registers.h."""
    B, N, D = _chk_reg(dtokens, R, dcls, dreg, dpos, mask, dmask_token, "embed_finish_reg_bwd", "dmask_token")
    dpatch = dpatch if dpatch is not None else torch.empty((B * N, D), dtype=out_dtype, device=dtokens.device)
    if dpatch.numel() != B * N * D:
        raise _cabi.VitError("embed_finish_reg_bwd: dpatch must hold [B*N, D]")
    p, seed, site = dropout
    _h(dtokens).call("vit_embed_finish_reg_bwd", dtokens.data_ptr(), _ptr(mask), dpatch.data_ptr(), _DT[dpatch.dtype], dcls.data_ptr(),
                     _ptr(dreg if R > 0 else None), _ptr(dpos), _ptr(dmask_token), B, R, N, D, p, seed, site, int(accumulate),
                     _stream(dtokens))
    return dpatch


def _chk_mim(x, pred, mask, P: int, who: str):
    _chk(x, torch.float32, who + " x")
    B, L = x.shape
    N = mask.shape[1]
    _chk_index(mask, B, N, who + " mask")
    if pred.dtype not in _DT or not pred.is_contiguous() or pred.numel() != B * (N + 1) * P:
        raise _cabi.VitError(f"{who}: pred must be a contiguous f32 / bf16 tensor holding [B*(N+1)={B * (N + 1)}, P={P}]")
    return B, L, N


def mim_loss_fwd(x, pred, mask, P: int, S: int, kind: int, norm_target: bool = False, loss=None, count=None):
    """(loss f32 [], count int32 []): the masked reconstruction loss of pred [B * (N + 1), P] against the windows of x [B, L]
    (vit_mim_loss_fwd); count = the number of masked windows, the loss's denominator / P."""
    B, L, N = _chk_mim(x, pred, mask, P, "mim_loss_fwd")
    loss = loss if loss is not None else torch.empty((), dtype=torch.float32, device=x.device)
    count = count if count is not None else torch.empty((), dtype=torch.int32, device=x.device)
    _chk(loss, torch.float32, "mim_loss_fwd loss")
    _chk(count, torch.int32, "mim_loss_fwd count")
    _h(x).call("vit_mim_loss_fwd", x.data_ptr(), pred.data_ptr(), _DT[pred.dtype], mask.data_ptr(), loss.data_ptr(),
               count.data_ptr(), B, L, P, S, N, N + 1, kind, int(bool(norm_target)), _stream(x))
    return loss, count


def mim_loss_bwd(x, pred, mask, count, dloss, P: int, S: int, kind: int, norm_target: bool = False, dpred=None,
                 out_dtype=torch.float32):
    """dpred [B * (N + 1), P] (dtype of the buffer): zeros in CLS and unmasked rows (vit_mim_loss_bwd)."""
    B, L, N = _chk_mim(x, pred, mask, P, "mim_loss_bwd")
    _chk(count, torch.int32, "mim_loss_bwd count")
    _chk(dloss, torch.float32, "mim_loss_bwd dloss")
    dpred = dpred if dpred is not None else torch.empty((B * (N + 1), P), dtype=out_dtype, device=x.device)
    if dpred.dtype not in _DT or not dpred.is_contiguous() or dpred.numel() != B * (N + 1) * P:
        raise _cabi.VitError("mim_loss_bwd: dpred must be a contiguous f32 / bf16 tensor holding [B*(N+1), P]")
    _h(x).call("vit_mim_loss_bwd", x.data_ptr(), pred.data_ptr(), _DT[pred.dtype], mask.data_ptr(), count.data_ptr(),
               dloss.data_ptr(), dpred.data_ptr(), _DT[dpred.dtype], B, L, P, S, N, N + 1, kind, int(bool(norm_target)), _stream(x))
    return dpred


# ------------------------------------------------------------------------------------------------ global average pooling
def _chk_pool(x, pooled, first: int, who: str):
    _chk(x, torch.float32, who + " x")
    _chk(pooled, torch.float32, who + " pooled")
    if x.dim() != 3 or not x.is_cuda or not pooled.is_cuda:
        raise _cabi.VitError(f"{who}: x must be an f32 [B, T, D] device tensor, got {tuple(x.shape)} on {x.device}")
    B, T, D = x.shape
    if pooled.numel() != B * D:
        raise _cabi.VitError(f"{who}: pooled must hold [B={B}, D={D}], got {tuple(pooled.shape)}")
    return B, T, D, int(first)


def token_pool_fwd(x, first: int = 1, out=None):
    """out f32 [B, D] <- the mean of rows first .. T-1 of x f32 [B, T, D], in the fixed order of include/vit_amd_pool.h
    (vit_token_pool_fwd)."""
    out = out if out is not None else torch.empty((x.shape[0], x.shape[2]), dtype=torch.float32, device=x.device)
    B, T, D, first = _chk_pool(x, out, first, "token_pool_fwd")
    _h(x).call("vit_token_pool_fwd", x.data_ptr(), out.data_ptr(), B, T, D, first, _stream(x))
    return out


def token_pool_bwd(dpooled, dx, first: int = 1):
    """dx f32 [B, T, D] <- dpooled [B, D] / (T - first) in rows first .. T-1, exact zeros in front: every element is written
    (vit_token_pool_bwd)."""
    B, T, D, first = _chk_pool(dx, dpooled, first, "token_pool_bwd")
    _h(dx).call("vit_token_pool_bwd", dpooled.data_ptr(), dx.data_ptr(), B, T, D, first, _stream(dx))
    return dx


# ------------------------------------------------------------------------------------------------ elementwise
def dropout_bwd_cast(dx, dropout: Dropout = NO_DROP, out=None, out_dtype=torch.bfloat16):
    _chk(dx, torch.float32, "dropout_bwd_cast dx")
    h = _h(dx)
    cols = dx.shape[-1]
    rows = dx.numel() // cols
    out = out if out is not None else torch.empty(dx.shape, dtype=out_dtype, device=dx.device)
    p, seed, site = dropout
    h.call("vit_dropout_bwd_cast", dx.data_ptr(), out.data_ptr(), _DT[out.dtype], rows, cols, p, seed, site, _stream(dx))
    return out


def colsum(a, out=None, accumulate: bool = False):
    h = _h(a)
    rows, cols = a.shape
    out = out if out is not None else torch.empty(cols, dtype=torch.float32, device=a.device)
    h.call("vit_colsum", a.data_ptr(), _DT[a.dtype], a.stride(0), out.data_ptr(), rows, cols, int(accumulate), _stream(a))
    return out


# ------------------------------------------------------------------------------------------------ covariance statistics
def cov_accumulate(x, mean, acc, *, rows: Optional[int] = None, cols: Optional[int] = None):
    """acc[L, L] += (x - mean)^T (x - mean) over x's rows, upper 128 x 128 tiles only (vit_cov_accumulate).  x: f32 [n, >= L]
    with unit column stride, used in place through its row stride; mean: f32 with at least L elements."""
    h = _h(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise _cabi.VitError("cov_accumulate: x must be a 2-D f32 tensor with unit column stride")
    _chk(mean, torch.float32, "cov_accumulate mean")
    _chk(acc, torch.float32, "cov_accumulate acc")
    n = x.shape[0] if rows is None else rows
    L = x.shape[1] if cols is None else cols
    if n > x.shape[0] or L > x.shape[1] or mean.numel() < L or tuple(acc.shape) != (L, L):
        raise _cabi.VitError(f"cov_accumulate: x {tuple(x.shape)}, mean {mean.numel()}, acc {tuple(acc.shape)} do not fit n={n} L={L}")
    h.call("vit_cov_accumulate", x.data_ptr(), x.stride(0) if n > 1 else max(L, x.stride(0)), mean.data_ptr(),
           acc.data_ptr(), n, L, _stream(x))
    return acc


def cov_mean_finish(colsum, n_total: int, cols: Optional[int] = None):
    """colsum[:L] /= n_total in place (vit_cov_mean_finish): column sums -> the mean."""
    _chk(colsum, torch.float32, "cov_mean_finish colsum")
    h = _h(colsum)
    h.call("vit_cov_mean_finish", colsum.data_ptr(), colsum.numel() if cols is None else cols, int(n_total),
           _stream(colsum))
    return colsum


def cov_finish(acc, n_total: int, out=None):
    """cov = acc / (n_total - 1), lower triangle mirrored from the upper: bitwise symmetric (vit_cov_finish)."""
    _chk(acc, torch.float32, "cov_finish acc")
    h = _h(acc)
    L = acc.shape[0]
    out = out if out is not None else torch.empty((L, L), dtype=torch.float32, device=acc.device)
    _chk(out, torch.float32, "cov_finish out")
    h.call("vit_cov_finish", acc.data_ptr(), out.data_ptr(), L, int(n_total), _stream(acc))
    return out


def cast_f32_bf16(src, out=None):
    _chk(src, torch.float32, "cast_f32_bf16 src")
    h = _h(src)
    out = out if out is not None else torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    h.call("vit_cast_f32_bf16", src.data_ptr(), out.data_ptr(), src.numel(), _stream(src))
    return out


def cast_bf16_f32(src, out, scale: float = 1.0):
    """out (f32) = scale * src (bf16)."""
    _chk(src, torch.bfloat16, "cast_bf16_f32 src")
    _chk(out, torch.float32, "cast_bf16_f32 out")
    h = _h(src)
    h.call("vit_cast_bf16_f32", src.data_ptr(), out.data_ptr(), src.numel(), float(scale), _stream(src))
    return out


# ------------------------------------------------------------------------------------------------ head + loss
def head_loss_fwd(last_hidden, W, b, labels, loss_kind: int, logits=None, loss=None):
    _chk(last_hidden, torch.float32, "head_loss_fwd last_hidden")
    h = _h(last_hidden)
    B, T, D = last_hidden.shape
    Cn = W.shape[0]
    logits = logits if logits is not None else torch.empty((B, Cn), dtype=torch.float32, device=last_hidden.device)
    _chk(logits, torch.float32, "head_loss_fwd logits")
    if logits.numel() != B * Cn:
        raise _cabi.VitError("head_loss_fwd: logits must hold [B, C]")
    if labels is None:
        loss = None
    elif loss is None:
        loss = torch.zeros((), dtype=torch.float32, device=last_hidden.device)
    else:
        _chk(loss, torch.float32, "head_loss_fwd loss")
    h.call("vit_head_loss_fwd", last_hidden.data_ptr(), W.data_ptr(), b.data_ptr(), _ptr(labels), logits.data_ptr(),
           _ptr(loss), B, T, D, Cn, loss_kind, _stream(last_hidden))
    return logits, loss


def head_loss_bwd(last_hidden, W, logits, labels, dloss, loss_kind: int, dlast=None, dW=None, db=None):
    h = _h(last_hidden)
    B, T, D = last_hidden.shape
    Cn = W.shape[0]
    dlast = dlast if dlast is not None else torch.empty_like(last_hidden)
    dW = dW if dW is not None else torch.empty_like(W)
    db = db if db is not None else torch.empty(Cn, dtype=torch.float32, device=W.device)
    h.call("vit_head_loss_bwd", last_hidden.data_ptr(), W.data_ptr(), logits.data_ptr(), labels.data_ptr(),
           dloss.data_ptr(), dlast.data_ptr(), dW.data_ptr(), db.data_ptr(), B, T, D, Cn, loss_kind, 0,
           _stream(last_hidden))
    return dlast, dW, db


# ------------------------------------------------------------------------------------------------ optimizer
def grad_sqnorm(g, out=None, accumulate: bool = False):
    """out[0] = sum g^2 (accumulate: += ), deterministic two-stage reduction."""
    _chk(g, torch.float32, "grad_sqnorm g")
    h = _h(g)
    out = out if out is not None else torch.empty(1, dtype=torch.float32, device=g.device)
    h.call("vit_grad_sqnorm_acc" if accumulate else "vit_grad_sqnorm", g.data_ptr(), g.numel(), out.data_ptr(), _stream(g))
    return out


def adamw_step(p, g, m, v, p_bf16, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, sqnorm=None,
               max_norm=0.0, n: Optional[int] = None):
    h = _h(p)
    n = p.numel() if n is None else n
    h.call("vit_adamw_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(p_bf16), n, lr, beta1, beta2, eps,
           weight_decay, step, _ptr(sqnorm), max_norm, _stream(p))


def adam_l2_step(p, g, m, v, p_bf16, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, sqnorm=None,
                 max_norm=0.0, n: Optional[int] = None):
    """torch.optim.Adam with weight_decay as L2 in the (clipped) gradient; otherwise `adamw_step`."""
    h = _h(p)
    n = p.numel() if n is None else n
    h.call("vit_adam_l2_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(p_bf16), n, lr, beta1, beta2, eps,
           weight_decay, step, _ptr(sqnorm), max_norm, _stream(p))


def sgd_step(p, g, buf, p_bf16, *, lr, momentum=0.0, weight_decay=0.0, nesterov=False, sqnorm=None, max_norm=0.0,
             n: Optional[int] = None):
    """torch.optim.SGD (dampening 0) over a flat buffer; `buf` (the momentum buffer) may be None when momentum == 0."""
    h = _h(p)
    n = p.numel() if n is None else n
    h.call("vit_sgd_step", p.data_ptr(), g.data_ptr(), _ptr(buf), _ptr(p_bf16), n, lr, momentum, weight_decay, int(bool(nesterov)),
           _ptr(sqnorm), max_norm, _stream(p))


# ------------------------------------------------------------------------------------------------ optimizer: parameter groups
class GroupTables:
    """The two device tables of the `*_step_groups` kernels (include/vit_amd_optim.h): `seg_end` (int64) / `seg_group` (int32),
    one entry per segment, and `groups`, one f32 row {lr, weight_decay, momentum, 0} per group.  `values` mirrors on the host
    what `groups` holds (None: nothing written yet), so that `optim_groups_write` launches only for a changed number."""

    def __init__(self, seg_end, seg_group, groups):
        self.seg_end, self.seg_group, self.groups = seg_end, seg_group, groups
        self.n_segments, self.n_groups = seg_end.numel(), groups.shape[0]
        self.values = None


def optim_group_tables(triples, n_groups: int, device, total: Optional[int] = None) -> GroupTables:
    """Build and validate the tables from (offset, numel, group) triples: sorted by offset, not overlapping, every offset and
    every end a multiple of 4 (the last end may instead equal `total`, the buffer's length), group indices in
    [0, n_groups).  Neighbouring triples of one group become one segment; a gap between two triples (parameters no group
    owns, which no step covers) falls to the segment behind it."""
    triples = [(int(o), int(k), int(gi)) for o, k, gi in triples]
    if not triples or n_groups <= 0:
        raise ValueError("optim_group_tables: needs at least one (offset, numel, group) triple and one group")
    ends, owners, prev_end = [], [], 0
    for i, (off, numel, gi) in enumerate(triples):
        if off < 0 or numel <= 0:
            raise ValueError(f"optim_group_tables: triple {i} = ({off}, {numel}, {gi}) is empty or negative")
        if off < prev_end:
            raise ValueError(f"optim_group_tables: triple {i} starts at {off}, before the end {prev_end} of the one in front "
                             f"(triples must be sorted by offset and must not overlap)")
        if not 0 <= gi < n_groups:
            raise ValueError(f"optim_group_tables: triple {i} names group {gi}, outside [0, {n_groups})")
        end = off + numel
        last = i == len(triples) - 1
        if off % 4 or (end % 4 and not (last and (total is None or end == total))):
            raise ValueError(f"optim_group_tables: triple {i} = [{off}, {end}) is not aligned to 4 elements (only the last "
                             f"end may be, when it is the buffer's length)")
        if total is not None and end > total:
            raise ValueError(f"optim_group_tables: triple {i} ends at {end}, past the buffer's length {total}")
        if owners and owners[-1] == gi and off == prev_end:
            ends[-1] = end
        else:
            ends.append(end)
            owners.append(gi)
        prev_end = end
    return GroupTables(torch.tensor(ends, dtype=torch.int64, device=device), torch.tensor(owners, dtype=torch.int32, device=device),
                       torch.zeros(n_groups, 4, dtype=torch.float32, device=device))


def optim_groups_write(tables: GroupTables, values) -> bool:
    """`values`: one (lr, weight_decay, momentum) per group.  Writes the device table on the current stream when a number
    differs from what it holds (vit_optim_groups_write: the numbers travel in kernel arguments); returns whether it did."""
    values = [(float(a), float(b), float(c)) for a, b, c in values]
    if len(values) != tables.n_groups:
        raise ValueError(f"optim_groups_write: {len(values)} rows for a table of {tables.n_groups} groups")
    if values == tables.values:
        return False
    arr = (C.c_float * (3 * len(values)))(*[x for row in values for x in row])
    _h(tables.groups).call("vit_optim_groups_write", tables.groups.data_ptr(), len(values), arr, _stream(tables.groups))
    tables.values = values
    return True


def _groups_args(tables: GroupTables, base: int):
    return int(base), tables.seg_end.data_ptr(), tables.seg_group.data_ptr(), tables.n_segments, tables.groups.data_ptr(), tables.n_groups


def adamw_step_groups(p, g, m, v, p_bf16, tables: GroupTables, *, base=0, beta1=0.9, beta2=0.999, eps=1e-8, step=1, sqnorm=None,
                      max_norm=0.0, n: Optional[int] = None, l2: bool = False, dyn: bool = False):
    """`adamw_step` (`l2`: `adam_l2_step`) over p = buffer[base : base + n] with each element's group's lr / weight_decay.
    `dyn` (inside a captured step): the bias corrections come from the handle's bound record instead of `step`."""
    h = _h(p)
    n = p.numel() if n is None else n
    name = ("vit_adam_l2_step_groups" if l2 else "vit_adamw_step_groups") + ("_dyn" if dyn else "")
    h.call(name, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(p_bf16), n, *_groups_args(tables, base), beta1, beta2,
           eps, *(() if dyn else (step,)), _ptr(sqnorm), max_norm, _stream(p))


def adam_l2_step_groups(p, g, m, v, p_bf16, tables: GroupTables, **kw):
    adamw_step_groups(p, g, m, v, p_bf16, tables, l2=True, **kw)


def sgd_step_groups(p, g, buf, p_bf16, tables: GroupTables, *, base=0, nesterov=False, sqnorm=None, max_norm=0.0,
                    n: Optional[int] = None, dyn: bool = False):
    """`sgd_step` over p = buffer[base : base + n] with each element's group's lr / momentum / weight_decay; `buf` may be None
    when every group's momentum is 0.  `dyn` (inside a captured step): insists on the handle's bound record."""
    h = _h(p)
    n = p.numel() if n is None else n
    h.call("vit_sgd_step_groups_dyn" if dyn else "vit_sgd_step_groups", p.data_ptr(), g.data_ptr(), _ptr(buf), _ptr(p_bf16), n,
           *_groups_args(tables, base), int(bool(nesterov)), _ptr(sqnorm), max_norm, _stream(p))


# ------------------------------------------------------------------------------------------------ optimizer: LAMB
LAMB_TILE = 4096  # VIT_LAMB_TILE (include/vit_amd_optim.h): elements per tile of the norms, cut from each segment's start


class ParamTables(GroupTables):
    """`GroupTables` with one segment per parameter tensor, as LAMB's per-tensor norms need them (`optim_param_tables`).
    `starts` / `ends` / `owners` mirror the segment table on the host (owner -1: a gap no group owns, a segment of its own);
    `segment_of[i]` is the segment number of the i-th triple the table was built from."""

    def __init__(self, seg_end, seg_group, groups, starts, ends, owners, segment_of):
        super().__init__(seg_end, seg_group, groups)
        self.starts, self.ends, self.owners, self.segment_of = starts, ends, owners, segment_of

    def check_run(self, base: int, n: int):
        """A LAMB call covers whole segments: `base` and `base + n` are segment boundaries, else ValueError."""
        base, n = int(base), int(n)
        bounds = set(self.starts) | set(self.ends)
        if n <= 0 or base not in bounds or base + n not in bounds:
            raise ValueError(f"lamb_step_groups: the run [{base}, {base + n}) cuts a parameter tensor; a trust ratio is a norm "
                             f"over a whole tensor, so a run starts and ends on segment boundaries")


def optim_param_tables(triples, n_groups: int, device, total: Optional[int] = None) -> ParamTables:
    """`optim_group_tables` without the merging: every (offset, numel, group) triple -- one parameter tensor with its alignment
    pad -- is a segment of its own, whoever owns its neighbours, and a gap between two triples (or in front of the first) is a
    segment of its own with group index -1, which the LAMB kernels neither read nor write.  Same validation."""
    checked = optim_group_tables(triples, n_groups, "cpu", total)  # the validation, stated once (its tables are dropped)
    del checked
    starts, ends, owners, segment_of, prev_end = [], [], [], [], 0
    for off, numel, gi in ((int(o), int(k), int(gi)) for o, k, gi in triples):
        if off > prev_end:
            starts.append(prev_end); ends.append(off); owners.append(-1)
        segment_of.append(len(ends))
        starts.append(off); ends.append(off + numel); owners.append(gi)
        prev_end = off + numel
    return ParamTables(torch.tensor(ends, dtype=torch.int64, device=device), torch.tensor(owners, dtype=torch.int32, device=device),
                       torch.zeros(n_groups, 4, dtype=torch.float32, device=device), starts, ends, owners, segment_of)


def lamb_step(p, g, m, v, p_bf16, *, lr, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.0, always_adapt=False,
              trust_clip=False, step=1, sqnorm=None, max_norm=0.0, trust=None, n: Optional[int] = None):
    """LAMB on one tensor, by value (include/vit_amd_optim.h); `trust` (one f32, optional) receives the tensor's trust ratio."""
    h = _h(p)
    n = p.numel() if n is None else n
    h.call("vit_lamb_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(p_bf16), n, lr, beta1, beta2, eps,
           weight_decay, int(bool(always_adapt)), int(bool(trust_clip)), step, _ptr(sqnorm), max_norm, _ptr(trust), _stream(p))


def lamb_step_groups(p, g, m, v, p_bf16, tables: ParamTables, trust, *, base=0, beta1=0.9, beta2=0.999, eps=1e-6,
                     always_adapt=False, trust_clip=False, step=1, sqnorm=None, max_norm=0.0, n: Optional[int] = None,
                     dyn: bool = False):
    """LAMB over p = buffer[base : base + n], whole segments of the per-parameter table (a run that cuts one: ValueError), with
    each tensor's group's lr / weight_decay; `trust` (f32, `tables.n_segments` entries) receives the ratios of the run's
    segments.  `dyn` (inside a captured step): the bias corrections come from the handle's bound record instead of `step`."""
    n = p.numel() if n is None else n
    if not isinstance(tables, ParamTables):
        raise ValueError("lamb_step_groups needs the per-parameter tables (optim_param_tables): merged runs would merge the norms")
    tables.check_run(base, n)
    _chk(trust, torch.float32, "lamb_step_groups trust")
    if trust.numel() < tables.n_segments:
        raise ValueError(f"lamb_step_groups: trust holds {trust.numel()} entries for {tables.n_segments} segments")
    _h(p).call("vit_lamb_step_groups_dyn" if dyn else "vit_lamb_step_groups", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
           _ptr(p_bf16), n, *_groups_args(tables, base), beta1, beta2, eps, int(bool(always_adapt)), int(bool(trust_clip)),
           *(() if dyn else (step,)), _ptr(sqnorm), max_norm, trust.data_ptr(), _stream(p))


# ------------------------------------------------------------------------------------------------ optimizer: Muon
MUON_TILE = 4096      # VIT_MUON_TILE (include/vit_amd_muon.h): elements per streaming tile of the norm's partial sums
MUON_GEMM_TILE = 64   # VIT_MUON_GEMM_TILE: rows and columns of C per workgroup of the grouped product
_MUON_TT = 32         # the transposing tile of vit_muon_normalize / vit_muon_apply


def muon_adjust_ratio(mode: str, rows: int, cols: int) -> float:
    """torch.optim.Muon's `_adjust_lr` as the factor on lr, for a matrix [rows, cols]."""
    if mode == "original":
        return max(1.0, rows / cols) ** 0.5
    if mode == "match_rms_adamw":
        return 0.2 * max(rows, cols) ** 0.5
    if mode in (None, "none"):
        return 1.0
    raise ValueError(f"muon adjust_lr = {mode!r}: expected 'match_rms_adamw', 'original' or 'none'")


def _device_bytes(array, device):
    return torch.frombuffer(bytearray(bytes(array)), dtype=torch.uint8).to(device)


class MuonTables:
    """The device table of vit_muon_mat entries (include/vit_amd_muon.h) with its host mirror: `entries` = [(off, xoff, rows,
    cols, group, ratio)], `n_tiles` / `n_ttiles` the totals of streaming / transposing tiles."""

    def __init__(self, mats, entries, n_tiles, n_ttiles):
        self.mats, self.entries, self.n_mats, self.n_tiles, self.n_ttiles = mats, entries, len(entries), n_tiles, n_ttiles

    def check_run(self, base: int, n: int):
        """A Muon call covers whole matrices: one of the table's that the run [base, base + n) cuts is a ValueError."""
        muon_check_run([(off, rows, cols) for off, _, rows, cols, _, _ in self.entries], base, n)


def muon_check_run(mats, base: int, n: int):
    """`mats`: (off, rows, cols) of the matrices a run [base, base + n) of the flat buffer is to step.  The orthogonalisation is a
    function of a whole matrix, so a run that cuts one is a ValueError (the one statement of that rule: the table's `check_run`
    and FusedMuon's runs both come here)."""
    lo, hi = int(base), int(base) + int(n)
    for off, rows, cols in mats:
        if not (lo <= off and off + rows * cols <= hi):
            raise ValueError(f"muon: the run [{lo}, {hi}) cuts the matrix at [{off}, {off + rows * cols}); the orthogonalisation "
                             f"is a function of the whole matrix")


def muon_mat_table(entries, device, total: Optional[int] = None, compact_total: Optional[int] = None) -> MuonTables:
    """Build and validate the matrix table from (off, xoff, rows, cols, group, ratio): rows and cols multiples of 16 (the MFMA
    tiles' and the 16-byte accesses' granule), offsets multiples of 8 and non-negative, matrices overlapping neither in the flat
    buffer nor in the compact one, inside `total` / `compact_total` where given."""
    ents = [(int(o), int(x), int(r), int(c), int(gi), float(ratio)) for o, x, r, c, gi, ratio in entries]
    if not ents:
        raise ValueError("muon_mat_table: needs at least one matrix")
    arr = (_cabi.MuonMat * len(ents))()
    tile0 = ttile0 = 0
    for i, (off, xoff, rows, cols, gi, ratio) in enumerate(ents):
        if rows < 16 or cols < 16 or rows % 16 or cols % 16:
            raise ValueError(f"muon_mat_table: matrix {i} is [{rows}, {cols}]; both sizes must be multiples of 16, at least 16")
        if off < 0 or xoff < 0 or off % 8 or xoff % 8:
            raise ValueError(f"muon_mat_table: matrix {i}: offsets ({off}, {xoff}) must be non-negative multiples of 8")
        if gi < 0 or not ratio > 0:
            raise ValueError(f"muon_mat_table: matrix {i}: group {gi} / ratio {ratio}")
        if total is not None and off + rows * cols > total or compact_total is not None and xoff + rows * cols > compact_total:
            raise ValueError(f"muon_mat_table: matrix {i} ends past its buffer")
        arr[i] = _cabi.MuonMat(off, xoff, rows, cols, gi, ratio, tile0, ttile0, 0)
        tile0 += -(-rows * cols // MUON_TILE)
        ttile0 += -(-rows // _MUON_TT) * -(-cols // _MUON_TT)
    for key in (0, 1):
        spans = sorted((e[key], e[key] + e[2] * e[3]) for e in ents)
        if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
            raise ValueError("muon_mat_table: two matrices overlap")
    return MuonTables(_device_bytes(arr, device), ents, tile0, ttile0)


class MuonProblems:
    """The device tables of one vit_muon_gemm_grouped launch: vit_muon_problem entries and the (problem, tile row, tile column, 0)
    tile table.  `held` keeps the operand tensors alive: the table holds their addresses."""

    def __init__(self, problems, tiles, n_problems, n_tiles, b_trans, held, shapes):
        self.problems, self.tiles, self.n_problems, self.n_tiles = problems, tiles, n_problems, n_tiles
        self.b_trans, self.held, self.shapes = bool(b_trans), held, shapes


def _chk_muon_operand(t, shape, who):
    if t.dtype != torch.bfloat16 or t.ndim != 2 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: expected a bf16 matrix {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) % 8 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        raise ValueError(f"{who}: rows must be contiguous, the leading dimension a multiple of 8 and the pointer 16-byte aligned")


def muon_problem_table(problems, b_trans: bool, device) -> MuonProblems:
    """`problems`: [(A, B, R or None, C, alpha, beta)] of bf16 2-D views, C [m, n] = bf16(alpha * A op(B) + beta * R) with A [m, k]
    and B [n, k] (`b_trans`: A B^T) or [k, n] (A B).  m, n, k multiples of 16; C must alias no operand."""
    if not problems:
        raise ValueError("muon_problem_table: needs at least one problem")
    arr = (_cabi.MuonProblem * len(problems))()
    tiles, held, shapes = [], [], []
    for i, (A, B, R, Cm, alpha, beta) in enumerate(problems):
        m, k = A.shape
        n = B.shape[0] if b_trans else B.shape[1]
        who = f"muon_problem_table: problem {i}"
        if min(m, n, k) < 16 or m % 16 or n % 16 or k % 16:
            raise ValueError(f"{who}: (m, n, k) = ({m}, {n}, {k}) must be multiples of 16, at least 16")
        _chk_muon_operand(A, (m, k), who + " A")
        _chk_muon_operand(B, (n, k) if b_trans else (k, n), who + " B")
        _chk_muon_operand(Cm, (m, n), who + " C")
        if R is not None:
            _chk_muon_operand(R, (m, n), who + " R")
        if beta != 0 and R is None:
            raise ValueError(f"{who}: beta = {beta} needs R")
        c_lo, c_hi = Cm.data_ptr(), Cm.data_ptr() + 2 * ((m - 1) * Cm.stride(0) + n)
        for t in (A, B, R):
            if t is not None and t.data_ptr() < c_hi and c_lo < t.data_ptr() + 2 * ((t.shape[0] - 1) * t.stride(0) + t.shape[1]):
                raise ValueError(f"{who}: C overlaps an operand (other tiles still read it while one writes)")
        arr[i] = _cabi.MuonProblem(A.data_ptr(), B.data_ptr(), None if R is None else R.data_ptr(), Cm.data_ptr(), m, n, k,
                                   A.stride(0), B.stride(0), 0 if R is None else R.stride(0), Cm.stride(0), float(alpha),
                                   float(beta), 0)
        tiles += [(i, tr, tc, 0) for tr in range(-(-m // MUON_GEMM_TILE)) for tc in range(-(-n // MUON_GEMM_TILE))]
        held += [A, B, R, Cm]
        shapes.append((m, n, k))
    # the header's rule is table-wide: no C_i may overlap an operand -- or another output -- of ANY problem of the launch
    span = lambda t: (t.data_ptr(), t.data_ptr() + 2 * ((t.shape[0] - 1) * t.stride(0) + t.shape[1]))
    outs = sorted(span(p[3]) + (i,) for i, p in enumerate(problems))
    for (_, a_hi, i), (b_lo, _, j) in zip(outs, outs[1:]):
        if b_lo < a_hi:
            raise ValueError(f"muon_problem_table: the outputs of problems {i} and {j} overlap")
    reads = sorted({span(t) for p in problems for t in p[:3] if t is not None})
    for c_lo, c_hi, i in outs:
        for r_lo, r_hi in reads:  # ascending by start: nothing behind the first that starts at or past c_hi can overlap
            if r_lo >= c_hi:
                break
            if c_lo < r_hi:
                raise ValueError(f"muon_problem_table: C of problem {i} overlaps an operand of the launch (other tiles still "
                                 f"read it while one writes)")
    return MuonProblems(_device_bytes(arr, device), torch.tensor(tiles, dtype=torch.int32, device=device), len(problems), len(tiles),
                        b_trans, held, shapes)


def muon_gemm_grouped(table: MuonProblems):
    """Every problem of the table in one launch (vit_muon_gemm_grouped)."""
    _h(table.problems).call("vit_muon_gemm_grouped", table.problems.data_ptr(), table.n_problems, table.tiles.data_ptr(),
                            table.n_tiles, int(table.b_trans), _stream(table.problems))


def _chk_muon_compact(t, dtype, tables: MuonTables, name: str):
    _chk(t, dtype, name)
    need = max(x + r * c for _, x, r, c, _, _ in tables.entries)
    if t.numel() < need:
        raise ValueError(f"{name}: holds {t.numel()} elements, the table's matrices need {need}")


def muon_momentum(g, buf, u, tables: MuonTables, part, *, momentum=0.95, nesterov=True, sqnorm=None, max_norm=0.0):
    """buf <- lerp(buf, g * clip, 1 - momentum); u (bf16) <- the Nesterov (or plain) momentum; part[tile] <- sum bf16(u)^2 (f64).
    `g` is the flat gradient buffer from element 0 (the table's `off`), `buf` / `u` the compact ones (`xoff`)."""
    _chk(g, torch.float32, "muon_momentum g")
    _chk_muon_compact(buf, torch.float32, tables, "muon_momentum buf")
    _chk_muon_compact(u, torch.bfloat16, tables, "muon_momentum u")
    _chk(part, torch.float64, "muon_momentum part")
    if part.numel() < tables.n_tiles or g.numel() < max(o + r * c for o, _, r, c, _, _ in tables.entries):
        raise ValueError("muon_momentum: part or g is shorter than the table needs")
    _h(g).call("vit_muon_momentum", g.data_ptr(), buf.data_ptr(), u.data_ptr(), tables.mats.data_ptr(), tables.n_mats,
               tables.n_tiles, float(momentum), int(bool(nesterov)), _ptr(sqnorm), float(max_norm), part.data_ptr(), _stream(g))


def muon_norms(tables: MuonTables, part, inv_norm, norms, *, eps=1e-7):
    """norms[i] <- ||X0_i||_F and inv_norm[i] <- 1 / max(norm, eps), one wave per matrix over its tiles' partials."""
    _chk(part, torch.float64, "muon_norms part")
    _chk(inv_norm, torch.float32, "muon_norms inv_norm")
    _chk(norms, torch.float32, "muon_norms norms")
    if part.numel() < tables.n_tiles or min(inv_norm.numel(), norms.numel()) < tables.n_mats:
        raise ValueError("muon_norms: part, inv_norm or norms is shorter than the table needs")
    _h(part).call("vit_muon_norms", tables.mats.data_ptr(), tables.n_mats, part.data_ptr(), float(eps), inv_norm.data_ptr(),
                  norms.data_ptr(), _stream(part))


def muon_normalize(u, x, tables: MuonTables, inv_norm):
    """x (bf16, the wide orientation [m, n], m <= n) <- bf16(u * inv_norm), transposed where rows > cols."""
    _chk_muon_compact(u, torch.bfloat16, tables, "muon_normalize u")
    _chk_muon_compact(x, torch.bfloat16, tables, "muon_normalize x")
    _chk(inv_norm, torch.float32, "muon_normalize inv_norm")
    if inv_norm.numel() < tables.n_mats or u.data_ptr() == x.data_ptr():
        raise ValueError("muon_normalize: inv_norm is shorter than the table, or x aliases u")
    _h(u).call("vit_muon_normalize", u.data_ptr(), x.data_ptr(), tables.mats.data_ptr(), tables.n_mats, tables.n_ttiles,
               inv_norm.data_ptr(), _stream(u))


def muon_apply(p, p_bf16, o, tables: MuonTables, groups):
    """W <- W * (1 - lr * wd) - lr * ratio * O per matrix, O = `o` transposed back; `groups`: the f32 [n_groups, 4] group table."""
    _chk(p, torch.float32, "muon_apply p")
    _chk_muon_compact(o, torch.bfloat16, tables, "muon_apply o")
    _chk(groups, torch.float32, "muon_apply groups")
    need = max(off + r * c for off, _, r, c, _, _ in tables.entries)
    if p.numel() < need or (p_bf16 is not None and p_bf16.numel() < need):
        raise ValueError("muon_apply: p or p_bf16 is shorter than the table needs")
    if max(e[4] for e in tables.entries) >= groups.shape[0]:
        raise ValueError("muon_apply: a matrix names a group past the group table")
    _h(p).call("vit_muon_apply", p.data_ptr(), _ptr(p_bf16), o.data_ptr(), tables.mats.data_ptr(), tables.n_mats, tables.n_ttiles,
               groups.data_ptr(), groups.shape[0], _stream(p))


class MuonPlan:
    """Everything one orthogonalisation of a table's matrices launches: the workspaces (u / the two X, A, B -- bf16, owned here)
    and the three problem tables of an iteration for either parity of the X ping-pong.  `ns_steps` iterations are
    3 * ns_steps launches; the result lies in `result(ns_steps)`."""

    def __init__(self, tables: MuonTables, coefficients, device, x=None):
        a, b, c = (float(v) for v in coefficients)
        self.tables = tables
        n_x = max(xo + r * cl for _, xo, r, cl, _, _ in tables.entries)
        dims = [(min(r, cl), max(r, cl)) for _, _, r, cl, _, _ in tables.entries]
        n_a = sum(m * m for m, _ in dims)
        self.x = x if x is not None else [torch.zeros(n_x, dtype=torch.bfloat16, device=device) for _ in range(2)]
        self.A = torch.zeros(n_a, dtype=torch.bfloat16, device=device)
        self.B = torch.zeros(n_a, dtype=torch.bfloat16, device=device)
        gram, poly, upd = [[], []], [], [[], []]
        aoff = 0
        for (_, xo, _, _, _, _), (m, n) in zip(tables.entries, dims):
            X = [buf[xo:xo + m * n].view(m, n) for buf in self.x]
            Am, Bm = self.A[aoff:aoff + m * m].view(m, m), self.B[aoff:aoff + m * m].view(m, m)
            aoff += m * m
            poly.append((Am, Am, Am, Bm, c, b))                       # B = b A + c A A   (A A^T: A is symmetric)
            for par in (0, 1):
                gram[par].append((X[par], X[par], None, Am, 1.0, 0.0))     # A = X X^T
                upd[par].append((Bm, X[par], X[par], X[1 - par], 1.0, a))  # X' = a X + B X
        self.gram = [muon_problem_table(g, True, device) for g in gram]
        self.poly = muon_problem_table(poly, True, device)
        self.upd = [muon_problem_table(u, False, device) for u in upd]

    def iterate(self, ns_steps: int, start: int = 0):
        """`ns_steps` Newton-Schulz iterations from x[start]; returns the buffer the result lies in."""
        par = start
        for _ in range(int(ns_steps)):
            muon_gemm_grouped(self.gram[par])
            muon_gemm_grouped(self.poly)
            muon_gemm_grouped(self.upd[par])
            par ^= 1
        return self.x[par]


# ------------------------------------------------------------------------------------------------ weight averaging
def ema_update(ema, p, weight: float = 0.0, *, weight_dev=None, n: Optional[int] = None):
    """ema <- torch.lerp(ema, p, weight) over the first `n` elements (include/vit_amd_ema.h); `weight` is 1 - decay, already
    subtracted (in double: a Python float).  `weight_dev` (inside a captured step): the weight is read from that device cell."""
    _chk(ema, torch.float32, "ema_update ema")
    _chk(p, torch.float32, "ema_update p")
    n = p.numel() if n is None else n
    if n > min(ema.numel(), p.numel()):
        raise _cabi.VitError(f"ema_update: n = {n} exceeds a buffer ({ema.numel()}, {p.numel()} elements)")
    _h(p).call("vit_ema_update", ema.data_ptr(), p.data_ptr(), n, float(weight), _ptr(weight_dev), _stream(p))


def ema_swap(p, ema, p_bf16=None, *, n: Optional[int] = None):
    """Exchange the first `n` elements of p and ema in place; p_bf16 (optional) <- bf16 of the new p in the same pass."""
    _chk(ema, torch.float32, "ema_swap ema")
    _chk(p, torch.float32, "ema_swap p")
    n = p.numel() if n is None else n
    if n > min(ema.numel(), p.numel()) or (p_bf16 is not None and n > p_bf16.numel()):
        raise _cabi.VitError(f"ema_swap: n = {n} exceeds a buffer")
    if p_bf16 is not None:
        _chk(p_bf16, torch.bfloat16, "ema_swap p_bf16")
    _h(p).call("vit_ema_swap", p.data_ptr(), ema.data_ptr(), _ptr(p_bf16), n, _stream(p))


# ------------------------------------------------------------------------------------------------ sharpness-aware minimisation
def sam_sqnorm(g, p=None, *, adaptive: bool = False, accumulate: bool = False, out=None, n: Optional[int] = None):
    """out[0] (+)= sum (a_i g_i)^2 over the first `n` elements, a_i = |p_i| if adaptive else 1 (include/vit_amd_sam.h); the plain
    form does not read p and has grad_sqnorm's bits."""
    _chk(g, torch.float32, "sam_sqnorm g")
    n = g.numel() if n is None else n
    if adaptive:
        if p is None:
            raise _cabi.VitError("sam_sqnorm: the adaptive form needs p")
        _chk(p, torch.float32, "sam_sqnorm p")
    if n > g.numel() or (adaptive and n > p.numel()):
        raise _cabi.VitError(f"sam_sqnorm: n = {n} exceeds a buffer")
    out = out if out is not None else torch.empty(1, dtype=torch.float32, device=g.device)
    _chk(out, torch.float32, "sam_sqnorm out")
    _h(g).call("vit_sam_sqnorm", _ptr(p) if adaptive else None, g.data_ptr(), n, int(bool(adaptive)), int(bool(accumulate)),
               out.data_ptr(), _stream(g))
    return out


def sam_ascend(p, g, backup, p_bf16, rho: float, sqnorm, *, adaptive: bool = False, n: Optional[int] = None):
    """backup <- p; p <- p + c * g * rho / (sqrt(sqnorm[0]) + 1e-12), c = p^2 if adaptive else 1, over the first `n` elements;
    p_bf16 (optional) <- bf16 of the new p in the same pass.  `sqnorm` is a device scalar: nothing is synchronised."""
    for t, name in ((p, "p"), (g, "g"), (backup, "backup"), (sqnorm, "sqnorm")):
        _chk(t, torch.float32, f"sam_ascend {name}")
    n = p.numel() if n is None else n
    if n > min(p.numel(), g.numel(), backup.numel()) or (p_bf16 is not None and n > p_bf16.numel()) or sqnorm.numel() < 1:
        raise _cabi.VitError(f"sam_ascend: n = {n} exceeds a buffer")
    if p_bf16 is not None:
        _chk(p_bf16, torch.bfloat16, "sam_ascend p_bf16")
    _h(p).call("vit_sam_ascend", p.data_ptr(), g.data_ptr(), backup.data_ptr(), _ptr(p_bf16), n, float(rho), int(bool(adaptive)),
               sqnorm.data_ptr(), _stream(p))


def sam_descend(p, backup, p_bf16=None, *, n: Optional[int] = None):
    """p <- backup over the first `n` elements, bit for bit; p_bf16 (optional) <- bf16 of it in the same pass."""
    _chk(p, torch.float32, "sam_descend p")
    _chk(backup, torch.float32, "sam_descend backup")
    n = p.numel() if n is None else n
    if n > min(p.numel(), backup.numel()) or (p_bf16 is not None and n > p_bf16.numel()):
        raise _cabi.VitError(f"sam_descend: n = {n} exceeds a buffer")
    if p_bf16 is not None:
        _chk(p_bf16, torch.bfloat16, "sam_descend p_bf16")
    _h(p).call("vit_sam_descend", p.data_ptr(), backup.data_ptr(), _ptr(p_bf16), n, _stream(p))


# ------------------------------------------------------------------------------------------------ Mixup / CutMix
MIX_ROW_BYTES = 32  # vit_mix_row (include/vit_amd_mix.h)


def mix_plan_write(plan, rows):
    """Rows [0, len(rows)) of the device plan (uint8, 32 bytes a row, 16-byte aligned) <- `rows`: a sequence of
    (w, u, lo, hi, wy, uy).  The rows travel in kernel arguments on the current stream (vit_mix_plan_write)."""
    n = len(rows)
    if plan.dtype != torch.uint8 or not plan.is_contiguous() or plan.numel() < n * MIX_ROW_BYTES:
        raise _cabi.VitError(f"mix_plan_write: the plan must be a contiguous uint8 tensor of at least {n * MIX_ROW_BYTES} bytes")
    arr = (_cabi.MixRow * n)()
    for r, (w, u, lo, hi, wy, uy) in zip(arr, rows):
        r.w, r.u, r.lo, r.hi, r.wy, r.uy = float(w), float(u), int(lo), int(hi), float(wy), float(uy)
    _h(plan).call("vit_mix_plan_write", plan.data_ptr(), n, arr, _stream(plan))


def mix_signal(x, plan, n_rows: int, out=None):
    """Mixup / CutMix of x [B, L] (f32) by the device plan (vit_mix_signal); `out is x`: in place, None: a fresh tensor."""
    _chk(x, torch.float32, "mix_signal x")
    if x.dim() != 2:
        raise _cabi.VitError(f"mix_signal: x must be [B, L], got {tuple(x.shape)}")
    out = out if out is not None else torch.empty_like(x)
    _chk(out, torch.float32, "mix_signal out")
    if out.shape != x.shape:
        raise _cabi.VitError(f"mix_signal: out {tuple(out.shape)} is not shaped like x {tuple(x.shape)}")
    B, L = x.shape
    _h(x).call("vit_mix_signal", x.data_ptr(), out.data_ptr(), plan.data_ptr(), int(n_rows), B, L, _stream(x))
    return out


def mix_targets(labels, plan, n_rows: int, num_classes: Optional[int] = None, on: float = 1.0, off: float = 0.0, out=None):
    """The mixed labels of a batch (vit_mix_targets).  `num_classes` None: regression labels f32 [B] / [B, k], mixed linearly
    into a tensor of their shape; else class labels int64 [B] -> soft targets f32 [B, num_classes] over the smoothed one-hot
    rows (`on` at the label, `off` elsewhere)."""
    if not labels.is_contiguous():
        raise _cabi.VitError("mix_targets: labels must be contiguous")
    B = labels.shape[0]
    if num_classes is None:
        _chk(labels, torch.float32, "mix_targets labels")
        kind, Cn, shape = _cabi.MIX_LABELS_F32, labels.numel() // max(B, 1), labels.shape
    else:
        _chk(labels, torch.int64, "mix_targets labels")
        if labels.dim() != 1:
            raise _cabi.VitError(f"mix_targets: class labels must be [B], got {tuple(labels.shape)}")
        kind, Cn, shape = _cabi.MIX_LABELS_I64, int(num_classes), (B, int(num_classes))
    out = out if out is not None else torch.empty(shape, dtype=torch.float32, device=labels.device)
    _chk(out, torch.float32, "mix_targets out")
    if out.numel() != B * Cn:
        raise _cabi.VitError(f"mix_targets: out has {out.numel()} elements, expected {B * Cn}")
    _h(labels).call("vit_mix_targets", labels.data_ptr(), kind, out.data_ptr(), plan.data_ptr(), int(n_rows), B, Cn, float(on),
                    float(off), _stream(labels))
    return out


# ------------------------------------------------------------------------------------------------ LayerScale
class LayerScaleTable:
    """The device table of `vit_layer_scale_fold` / `vit_layer_scale_grad` (include/vit_amd_layerscale.h): 96 bytes per matrix.
    `rows[i]` mirrors entry i's row count on the host (the launch geometry); `held` keeps the tensors the entries point to."""

    def __init__(self, table, rows, held):
        self.table, self.rows, self.held = table, rows, held
        self.n = len(rows)


_LS_FIELDS = ("W", "b", "lam", "Wf", "bf", "dW_raw", "db_raw", "dW", "db", "dlam")
_LS_DTYPES = (torch.float32, torch.bfloat16)


def layer_scale_table(entries, device) -> LayerScaleTable:
    """Build the table from one dict per matrix: W [rows, cols], b, lam (f32); Wf (bf16 / f32 like W), bf -- the fold's outputs;
    dW_raw, db_raw, dW, db, dlam (f32) -- what the gradient pass reads and writes.  Either output set may be absent.  The library
    checks the entries (vit_layer_scale_table_write) and writes them on the current stream."""
    arr = (_cabi.LayerScaleEntry * len(entries))()
    rows, held = [], []
    for i, ent in enumerate(entries):
        W = ent["W"]
        if W.dim() != 2:
            raise _cabi.VitError(f"layer_scale_table: entry {i}: W must be a matrix")
        r, c = W.shape
        for k in _LS_FIELDS:
            t = ent.get(k)
            if t is None:
                continue
            if k != "Wf":
                _chk(t, torch.float32, f"layer_scale_table entry {i} {k}")
            elif t.dtype not in _LS_DTYPES or not t.is_contiguous():
                raise _cabi.VitError(f"layer_scale_table: entry {i}: Wf must be a contiguous bf16 / f32 tensor")
            if t.device != W.device or t.numel() != (r * c if k in ("W", "Wf", "dW_raw", "dW") else r):
                raise _cabi.VitError(f"layer_scale_table: entry {i}: {k} does not match W's shape {r} x {c} (or its device)")
            setattr(arr[i], k, t.data_ptr())
            held.append(t)
        arr[i].rows, arr[i].cols = r, c
        rows.append(r)
    table = torch.zeros(max(1, len(entries)) * 12, dtype=torch.int64, device=device)
    _h(table).call("vit_layer_scale_table_write", table.data_ptr(), arr, len(entries), _stream(table))
    return LayerScaleTable(table, rows, held)


def _ls_span(tab: LayerScaleTable, first: int, count: Optional[int]):
    count = tab.n - first if count is None else count
    if first < 0 or count <= 0 or first + count > tab.n:
        raise _cabi.VitError(f"layer scale: entries [{first}, {first + count}) are not inside a table of {tab.n}")
    return tab.table.data_ptr() + 96 * first, count, max(tab.rows[first:first + count])


def layer_scale_fold(tab: LayerScaleTable, out_dtype, first: int = 0, count: Optional[int] = None):
    """Wf = diag(lam) W (stored as `out_dtype`: what the entries' Wf tensors are), bf = lam * b for `count` entries from `first`."""
    ptr, count, max_rows = _ls_span(tab, first, count)
    _h(tab.table).call("vit_layer_scale_fold", ptr, count, max_rows, _DT[out_dtype], _stream(tab.table))


def layer_scale_grad(tab: LayerScaleTable, accumulate: bool = False, first: int = 0, count: Optional[int] = None):
    """dW (+)= diag(lam) dW_raw, db (+)= lam * db_raw, dlam (+)= rowsum(dW_raw * W) + db_raw * b; db_raw is left zeroed."""
    ptr, count, max_rows = _ls_span(tab, first, count)
    _h(tab.table).call("vit_layer_scale_grad", ptr, count, max_rows, int(bool(accumulate)), _stream(tab.table))


def ema_weight_write(cell, weight: float):
    """cell[0, 0] <- weight on the current stream: `cell` is a one-row group table ([1, 4] f32) and the number travels by value
    in a kernel argument (vit_optim_groups_write), so a captured vit_ema_update that reads the cell sees it in stream order."""
    arr = (C.c_float * 3)(float(weight), 0.0, 0.0)
    _h(cell).call("vit_optim_groups_write", cell.data_ptr(), 1, arr, _stream(cell))
