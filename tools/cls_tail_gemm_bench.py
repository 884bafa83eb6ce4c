"""The CLS tail's launches at C3 (B 256, T 197, D 768, Fd 3072): its six vit_gemm products on the ping-pong core (gemm_core 1)
against the 128x128 core (0), and the three ordered weight gradients + the ordered column sums (no core choice) as the engine calls them."""
import sys, torch
sys.path.insert(0, ".")
from vit_amd import _cabi, functional as vf
dev = torch.device("cuda:0")
B, T, D, Fd = 256, 197, 768, 3072
M = B * T
bf = torch.bfloat16
g = torch.Generator(device="cuda").manual_seed(1)
R = lambda *s, dt=bf: (torch.randn(*s, device=dev, generator=g) * 0.05).to(dt)
ctx, Wo, W1, W2 = R(M, D), R(D, D), R(Fd, D), R(D, Fd)
bo, b1, b2 = R(D, dt=torch.float32), R(Fd, dt=torch.float32), R(D, dt=torch.float32)
cy, ch2, cg, cu = R(B, D), R(B, D), R(B, Fd), R(B, Fd)
cdy, cdU, cdh = R(B, D), R(B, Fd), R(B, D)
gW2, gW1, gWo = (torch.empty(D, Fd, device=dev), torch.empty(Fd, D, device=dev), torch.empty(D, D, device=dev))
gb1 = torch.empty(Fd, device=dev)
dctx = torch.zeros(M, D, device=dev, dtype=bf)
drop = (0.1, 1234, 5)
cases = {
    "out-proj fwd  256x768x768 lda=T*D drop": lambda: vf.gemm(ctx, Wo, M=B, N=D, K=D, lda=T * D, out=cy, bias=bo, dropout=drop, drop_row_stride=T),
    "FC1 fwd       256x3072x768 gelu+grad ": lambda: vf.gemm(ch2, W1, M=B, N=Fd, K=D, out=cg, bias=b1, act=vf.ACT_GELU_GRAD, aux_out=cu),
    "FC2 fwd       256x768x3072 drop      ": lambda: vf.gemm(cg, W2, M=B, N=D, K=Fd, out=cy, bias=b2, dropout=drop, drop_row_stride=T),
    "dX FC2        256x3072x768 *aux      ": lambda: vf.gemm(cdy, W2, M=B, N=Fd, K=D, b_trans=True, out=cdU, act=vf.ACT_MUL_AUX, aux_in=cu),
    "dX FC1        256x768x3072           ": lambda: vf.gemm(cdU, W1, M=B, N=D, K=Fd, b_trans=True, out=cdh),
    "dX out-proj   256x768x768 ldc=T*D    ": lambda: vf.gemm(cdy, Wo, M=B, N=D, K=D, b_trans=True, out=dctx, ldc=T * D),
}
def timeit(fn, n=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
lib = _cabi.load()
tot = {0: 0.0, 1: 0.0}
for name, fn in cases.items():
    row = []
    for core in (1, 0, 1, 0):
        _cabi.set_option("gemm_core", core)
        t = timeit(fn)
        row.append((core, t, lib.vit_last_gemm_kernel().decode()))
    pp, gen = min(r[1] for r in row if r[0] == 1), min(r[1] for r in row if r[0] == 0)
    tot[1] += pp; tot[0] += gen
    print(f"{name}: ping-pong {pp:7.1f} us ({row[0][2]})   128x128 {gen:7.1f} us ({row[1][2]})", flush=True)
Mp = -(-M // 256) * 256
ordered = {
    "dW FC2   dw_rows 768x3072 over 256 rows ": lambda: vf.linear_bwd_dw_rows(cdy, cg, gW2, row_stride=T, full_rows=Mp),
    "dW FC1   dw_rows 3072x768 over 256 rows ": lambda: vf.linear_bwd_dw_rows(cdU, ch2, gW1, row_stride=T, full_rows=Mp),
    "dW out   dw_rows 768x768 ldx=T*D        ": lambda: vf.linear_bwd_dw_rows(cdy, ctx, gWo, row_stride=T, full_rows=Mp, ldx=T * D),
    "db1      colsum_rows 256x3072           ": lambda: vf.colsum_rows(cdU, gb1, row_stride=T, full_rows=Mp),
    "(for comparison) dW FC2 as a K = 256 vit_gemm": lambda: vf.gemm(cdy, cg, M=D, N=Fd, K=B, a_trans=True, b_trans=True, out=gW2, split_k=1),
    "(for comparison) dW out as a K = 256 vit_gemm": lambda: vf.gemm(cdy, ctx, M=D, N=D, K=B, a_trans=True, b_trans=True, ldb=T * D, out=gWo, split_k=1),
}
_cabi.set_option("gemm_core", 1)
for name, fn in ordered.items():
    print(f"{name}: {min(timeit(fn), timeit(fn)):7.1f} us", flush=True)
print(f"sum: ping-pong {tot[1]:.1f} us, 128x128 {tot[0]:.1f} us (back-to-back launches, includes launch overhead)")
