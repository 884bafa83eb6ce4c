"""The library states each call's workspace need before it launches anything (include/vit_amd.h, the handle's comment).

No device here: with a NULL handle -- which has no workspace -- and made-up pointers, a call that claims its whole need first
returns VIT_ERR_WORKSPACE (-4) and vit_workspace_needed() is that need; a launch in front of the claim would come back as
VIT_ERR_HIP (-2).  The pointers are never dereferenced, which is only true where nothing can launch: every test skips on a
machine with a GPU (tests/test_workspace_gpu.py checks the same property there, on real buffers)."""
import ctypes

import pytest
import torch

P = 0x10000  # any 16-byte-aligned non-null address
F32, BF16 = 0, 1
WS = -4


@pytest.fixture(autouse=True)
def _no_device():
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only where no device exists to launch on")


@pytest.fixture(scope="module")
def lib():
    from vit_amd import _cabi

    return _cabi.load()


ACT_DGELU, ACT_GELU_GRAD = 2, 3


def gemm_desc(M, N, K, *, ab=BF16, c=F32, a_trans=1, b_trans=1, split_k=-1, colsum=False, bias=False, act=0, rope=None,
              accumulate=0, buf=lambda name, rows, cols, dtype: P):
    """A vit_gemm descriptor over dense operands; buf(name, rows, cols, dtype) -> the address of that tensor (here: made up)."""
    from vit_amd import _cabi

    d = _cabi.GemmDesc()
    d.M, d.N, d.K, d.a_trans, d.b_trans, d.ab_dtype = M, N, K, a_trans, b_trans, ab
    d.lda, d.ldb, d.ldc, d.ldaux = (M if a_trans else K), (N if b_trans else K), N, N
    d.A = buf("A", K if a_trans else M, d.lda, ab)
    d.B = buf("B", K if b_trans else N, d.ldb, ab)
    d.C, d.c_dtype = buf("C", M, N, c), c
    d.alpha, d.split_k, d.act, d.accumulate = 1.0, split_k, act, accumulate
    if colsum:
        d.colsum_out = buf("colsum_out", 1, N, F32)
    if bias:
        d.bias = buf("bias", 1, N, F32)
    if act == ACT_GELU_GRAD:
        d.aux_out = buf("aux_out", M, N, BF16)
    if act == ACT_DGELU:
        d.aux_in = buf("aux_in", M, N, BF16)
    if rope:
        d.rope_T, d.rope_dh, d.rope_cols = rope
        d.rope_cos, d.rope_sin = buf("rope_cos", d.rope_T, d.rope_dh // 2, F32), buf("rope_sin", d.rope_T, d.rope_dh // 2, F32)
    return d


def colsum_ws_bytes(rows, cols):
    """vit_colsum's partial rows (elementwise.hip), as the parent's error text printed them: 16 x 768 x 4 at 1024 x 768."""
    gx = -(-cols // 256)
    return max(1, min(-(-rows // 64), 2048 // gx)) * cols * 4


# the needed bytes the parent's own error texts named for these calls
def test_needs_the_parent_printed(lib):
    assert lib.vit_colsum(None, P, BF16, 768, P, 1024, 768, 0, None) == WS
    assert lib.vit_workspace_needed() == 49152
    assert b"vit_colsum: needs 49152 workspace bytes, have 0" in lib.vit_last_error()
    assert lib.vit_layernorm_bwd(None, P, BF16, P, P, P, P, None, P, P, P, 64, 768, None) == WS
    assert lib.vit_workspace_needed() == 24576
    assert lib.vit_embed_finish_bwd(None, P, P, BF16, P, P, 4, 9, 64, 0.0, 0, 0, 0, None) == WS
    assert lib.vit_workspace_needed() == 9216
    assert lib.vit_cov_accumulate(None, P, 128, P, P, 100000, 128, None) == WS
    assert lib.vit_workspace_needed() == 25624576


@pytest.mark.parametrize("M,N,K,ab,need,kernel", [
    (256, 256, 4096, BF16, 2097152, "ping-pong core"),
    (128, 128, 4096, BF16, 1048576, "generic core"),
    (128, 128, 4096, F32, 2097152, "x3 kernel"),
])
def test_split_k_slabs_of_each_core(lib, M, N, K, ab, need, kernel):
    d = gemm_desc(M, N, K, ab=ab)
    assert lib.vit_gemm(None, ctypes.byref(d), None) == WS, kernel
    assert lib.vit_workspace_needed() == need, kernel


def test_grad_sqnorm_and_head_loss(lib):
    n = 4096
    blocks = max(1, min((n // 4 + 1 + 255) // 256, 1024))  # grid_for(n / 4 + 1, 256, 1024)
    assert lib.vit_grad_sqnorm(None, P, n, P, None) == WS
    assert lib.vit_workspace_needed() == blocks * 4
    B, T, D, Cn = 4, 9, 64, 3
    assert lib.vit_head_loss_bwd(None, P, P, P, P, P, P, P, P, B, T, D, Cn, 0, 0, None) == WS
    assert lib.vit_workspace_needed() == B * Cn * 4


def test_attention_bwd_claims_its_partial_rows_before_the_kernel(lib):
    B, H, T, dh = 2, 4, 65, 64  # the pipelined form: AttnPlan::csum_rows = B * 8, one row per wave
    rc = lib.vit_attention_bwd(None, P, P, None, P, P, P, P, BF16, B, H, T, dh, 0.125, 0.0, 0, 0, P, None)
    assert rc == WS
    assert lib.vit_workspace_needed() == B * 8 * 3 * H * dh * 4


def test_colsum_rows_claims_before_any_launch(lib):
    assert lib.vit_colsum_rows(None, P, BF16, 256, P, 4, 256, 64, 256, None) == WS
    assert lib.vit_workspace_needed() == (256 // 128) * 256 * 4


def test_gemm_with_colsum_out(lib):
    """The claim is that of the column-sum route the plan takes, not the larger of both."""
    d = gemm_desc(512, 256, 256, c=BF16, a_trans=0, b_trans=1, split_k=0, colsum=True)  # ping-pong: sums in the epilogue
    assert lib.vit_gemm(None, ctypes.byref(d), None) == WS
    assert lib.vit_workspace_needed() == (512 // 256) * 2 * 256 * 4 == 4096
    d = gemm_desc(200, 64, 64, c=BF16, a_trans=0, b_trans=0, split_k=0, colsum=True)  # generic: a vit_colsum pass behind it
    assert lib.vit_gemm(None, ctypes.byref(d), None) == WS
    assert lib.vit_workspace_needed() == colsum_ws_bytes(200, 64) == 1024


# What the plan of one vit_gemm decides, asked without a device: a call with a need is refused (-4) and states it, one without
# gets as far as its launch (-2); either way vit_last_gemm_kernel() names the kernel planned.  A NULL handle sees 256 CUs.
# Needs and symbols are the parent commit's: the needs as it stated them (colsum_out: of the route it then took), the symbols as
# its library reported them after running each call on an MI355X with real buffers.
FWD, DX, DW = dict(a_trans=0, b_trans=0), dict(a_trans=0, b_trans=1), dict(a_trans=1, b_trans=1)
GEMM_TABLE = {
    # split-K on each core
    "dw_splitk_pingpong": (dict(M=256, N=256, K=4096, **DW), 2097152, "gemm3_kernel<1, 1, 7, 8>"),
    "dw_splitk_generic": (dict(M=128, N=128, K=4096, **DW), 1048576, "gemm_bf16_kernel<1, 1>"),
    "dw_splitk_x3": (dict(M=128, N=128, K=4096, ab=F32, **DW), 2097152, "gemm_f32x3_kernel<1, 1>"),
    # column sums: passed behind the generic epilogue (0) and the generic core, fused into epilogues 5 and 6
    "dx_f32_colsum_pass": (dict(M=256, N=256, K=64, split_k=0, colsum=True, **DX), 4096, "gemm3_kernel<0, 1, 0, 8>"),
    "generic_colsum_pass": (dict(M=200, N=64, K=64, c=BF16, split_k=0, colsum=True, **FWD), 1024, "gemm_bf16_kernel<0, 0>"),
    "dx_dgelu_colsum_fused": (dict(M=256, N=256, K=64, c=BF16, split_k=0, act=ACT_DGELU, colsum=True, **DX), 2048,
                              "gemm3_kernel<0, 1, 5, 8>"),
    "dx_colsum_fused": (dict(M=512, N=256, K=256, c=BF16, split_k=0, colsum=True, **DX), 4096, "gemm3_kernel<0, 1, 6, 8>"),
    # no workspace: epilogues 3, 4, 7, 8, the rope pass behind epilogue 3 at head_dim 128 and behind the generic core, x3
    "fwd_bias": (dict(M=256, N=256, K=64, c=BF16, split_k=0, bias=True, **FWD), 0, "gemm3_kernel<0, 0, 3, 8>"),
    "fwd_gelu_grad": (dict(M=256, N=256, K=64, c=BF16, split_k=0, bias=True, act=ACT_GELU_GRAD, **FWD), 0,
                      "gemm3_kernel<0, 0, 4, 8>"),
    "dw_one_slice": (dict(M=256, N=256, K=64, split_k=1, **DW), 0, "gemm3_kernel<1, 1, 7, 8>"),
    "dw_one_slice_accumulate": (dict(M=256, N=256, K=64, split_k=1, accumulate=1, **DW), 0, "gemm3_kernel<1, 1, 0, 8>"),
    "qk_rope_epilogue": (dict(M=256, N=256, K=64, c=BF16, split_k=0, bias=True, rope=(16, 64, 256), **FWD), 0,
                         "gemm3_kernel<0, 0, 8, 8>"),
    "qk_rope_pass_dh128": (dict(M=256, N=512, K=64, c=BF16, split_k=0, bias=True, rope=(16, 128, 256), **FWD), 0,
                           "gemm3_kernel<0, 0, 3, 8>"),
    "projection_generic_rope_pass": (dict(M=256, N=384, K=64, c=BF16, split_k=0, bias=True, rope=(16, 64, 256), **FWD), 0,
                                     "gemm_bf16_kernel<0, 0>"),
    "fwd_x3": (dict(M=64, N=64, K=64, ab=F32, split_k=0, **FWD), 0, "gemm_f32x3_kernel<0, 0>"),
}


@pytest.mark.parametrize("name", list(GEMM_TABLE))
def test_gemm_plan_table(lib, name):
    kw, need, symbol = GEMM_TABLE[name]
    d = gemm_desc(**kw)
    assert lib.vit_gemm(None, ctypes.byref(d), None) == (WS if need else -2), lib.vit_last_error()
    if need:
        assert lib.vit_workspace_needed() == need
    assert lib.vit_last_gemm_kernel().decode() == symbol


def test_gemm_argument_errors_come_before_the_claim(lib):
    d = gemm_desc(128, 128, 4096, split_k=4, bias=True)  # the parent claimed the four slabs first (-4), then refused the bias
    assert lib.vit_gemm(None, ctypes.byref(d), None) == -1
    assert b"split_k supports only alpha and an f32 C" in lib.vit_last_error()


def test_handle_free_entry_points_no_longer_reject_a_null_handle(lib):
    """vit_linear_bwd_dw_rows / vit_colsum_rows took a NULL handle for an argument error; like every other call they now get as
    far as their workspace claim (f32, row_stride > 1: the full product's split-K slabs on the x3 kernel)."""
    assert lib.vit_linear_bwd_dw_rows(None, P, 128, P, 128, F32, P, 4, 128, 128, 1024, 4096, None) == WS
    assert lib.vit_workspace_needed() == 2097152  # the 128 x 128 x 4096 x3 product of the table above
