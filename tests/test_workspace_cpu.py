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


def gemm_desc(M, N, K, *, ab=BF16, c=F32, a_trans=1, b_trans=1, split_k=-1, colsum=False):
    from vit_amd import _cabi

    d = _cabi.GemmDesc()
    d.M, d.N, d.K, d.a_trans, d.b_trans, d.ab_dtype = M, N, K, a_trans, b_trans, ab
    d.A, d.lda = P, M if a_trans else K
    d.B, d.ldb = P, N if b_trans else K
    d.C, d.ldc, d.c_dtype = P, N, c
    d.alpha, d.split_k = 1.0, split_k
    if colsum:
        d.colsum_out = P
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
    d = gemm_desc(512, 256, 256, c=BF16, a_trans=0, b_trans=1, split_k=0, colsum=True)  # ping-pong: sums in the epilogue
    assert lib.vit_gemm(None, ctypes.byref(d), None) == WS
    assert lib.vit_workspace_needed() >= (512 // 256) * 2 * 256 * 4
    d = gemm_desc(200, 64, 64, c=BF16, a_trans=0, b_trans=0, split_k=0, colsum=True)  # generic: a vit_colsum pass behind it
    assert lib.vit_gemm(None, ctypes.byref(d), None) == WS
    assert lib.vit_workspace_needed() >= colsum_ws_bytes(200, 64)


def test_handle_free_entry_points_no_longer_reject_a_null_handle(lib):
    """vit_linear_bwd_dw_rows / vit_colsum_rows took a NULL handle for an argument error; like every other call they now get as
    far as their workspace claim (f32, row_stride > 1: the full product's split-K slabs on the x3 kernel)."""
    assert lib.vit_linear_bwd_dw_rows(None, P, 128, P, 128, F32, P, 4, 128, 128, 1024, 4096, None) == WS
    assert lib.vit_workspace_needed() == 2097152  # the 128 x 128 x 4096 x3 product of the table above
