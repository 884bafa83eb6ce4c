#!/usr/bin/env python3
"""Rate of one vit_cov_accumulate (exact-f32 MFMA, upper tiles only) at n = 65536, L = 4096 and L = 1024, on random data.
FLOP counted: the algorithmic n L (L + 1) of a symmetric rank-k update.  Beside it, for context, the same product as a FULL
square X^T X through vf.gemm(..., a_trans=True) in the '32' form (split-bf16 x3 operands), counted 2 n L^2.  Device events
around `--iters` back-to-back calls after a warm-up; no gate, the numbers go into DESIGN.md with the box they came from.
Also times the host eigendecomposition (torch.linalg.eigh) of the L = 4096 covariance: finish_host's share.
Usage: python tools/cov_bench.py [--n 65536] [--iters 10] [--no-eigh]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import vit_amd.functional as vf
from vit_amd import covstats


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-eigh", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.n
    print(f"device: {torch.cuda.get_device_name(0)}; n = {n}, {args.iters} timed calls per figure")
    for L in (4096, 1024):
        torch.manual_seed(L)
        x = torch.randn(n, L, device=dev) + 1.0
        mean = vf.colsum(x)
        vf.cov_mean_finish(mean, n)
        acc = torch.zeros(L, L, device=dev)
        out = torch.empty(L, L, device=dev)
        ms = timed(lambda: vf.cov_accumulate(x, mean, acc), args.iters)
        ms_mean = timed(lambda: vf.colsum(x, out=mean), args.iters)
        ms_gemm = timed(lambda: vf.gemm(x, x, M=L, N=L, K=n, a_trans=True, b_trans=True, out=out, out_dtype=torch.float32,
                                        split_k=-1), args.iters)
        print(f"L = {L}: vit_cov_accumulate {ms:.2f} ms = {n * L * (L + 1) / ms * 1e-9:.1f} TFLOP/s (n L (L + 1) FLOP, exact f32); "
              f"column sums {ms_mean:.2f} ms = {n * L * 4 / ms_mean * 1e-9:.2f} TB/s; "
              f"full-square '32' vit_gemm (x3 split-bf16) {ms_gemm:.2f} ms = {2 * n * L * L / ms_gemm * 1e-9:.1f} TFLOP/s (2 n L^2 FLOP)")
        if L == 4096 and not args.no_eigh:
            cov = vf.cov_finish(acc, (args.iters + 2) * n).cpu()
            t = {}
            covstats.finish_host(mean.cpu(), cov, n, timings=t)
            print(f"L = 4096: host eigh (finish_host, {torch.get_num_threads()} threads) {t['eigh_s']:.2f} s")
        del x, acc, out


if __name__ == "__main__":
    main()
