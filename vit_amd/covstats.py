"""Covariance statistics of the training spectra: what `warmup.cov_path` names (`mean / cov / eigvals / eigvecs`), computed
here instead of taken from a file made elsewhere.  Reference: compute_covariance_stats / load_or_compute_covariance
(src/prepca/preprocessor_utils.py:399-531) and _sorted_eigh_sym (:44-62).

The O(n L^2) part runs on the MI355X through the C ABI, in two passes over row chunks (so a split larger than device memory
works): column sums (`vit_colsum(..., accumulate)`, then `vit_cov_mean_finish`), then the centred symmetric rank-k update on
exact-f32 MFMA (`vit_cov_accumulate`) and `vit_cov_finish`.  There is no CPU path for that part.  The eigendecomposition is
O(L^3) once per dataset and stays on the host (`finish_host`: torch.linalg.eigh, as the reference does); the product path
links no vendor solver.
"""
from __future__ import annotations

import os
import time
from typing import Optional

import torch

__all__ = ["compute_covariance_stats", "finish_host", "save", "ensure_cov_file"]


def finish_host(mean: torch.Tensor, cov: torch.Tensor, n: int, src_path=None, timings: Optional[dict] = None) -> dict:
    """The reference's payload from a mean and a covariance: _sorted_eigh_sym restated (symmetrise, torch.linalg.eigh on the
    CPU, clamp the eigenvalues at 0, sort descending).  Keys: mean [L], cov [L, L] (the symmetrised one), num_samples (0-dim
    int64), eigvals [L], eigvecs [L, L] (columns), all f32; src_path (str) when given.

    One thing the reference leaves to chance is pinned: the covariance of n samples has rank <= n - 1, so with n - 1 < L the
    eigenvalues from position n - 1 on are rounding noise of either sign around 0 (|lambda| ~ L 2^-24 lambda_0); the clamp
    zeroes the negative half of them, this sets all of them to exactly 0."""
    mean = mean.detach().to("cpu", torch.float32).contiguous()
    cov = cov.detach().to("cpu", torch.float32)
    L = int(mean.numel())
    if cov.shape != (L, L):
        raise ValueError(f"finish_host: cov {tuple(cov.shape)} does not match mean [{L}]")
    n = int(n)
    if n < 2:
        raise ValueError(f"covariance statistics need at least 2 samples (got {n})")
    t0 = time.perf_counter()
    cov_sym = (0.5 * (cov + cov.t())).contiguous()
    eigvals, eigvecs = torch.linalg.eigh(cov_sym)
    eigvals = torch.clamp(eigvals, min=0.0)
    idx = torch.argsort(eigvals, descending=True)
    eigvals, eigvecs = eigvals[idx].contiguous(), eigvecs[:, idx].contiguous()
    if n - 1 < L:
        eigvals[n - 1:] = 0.0
    if timings is not None:
        timings["eigh_s"] = time.perf_counter() - t0
    stats = {"mean": mean, "cov": cov_sym, "num_samples": torch.tensor(n), "eigvals": eigvals.to(torch.float32),
             "eigvecs": eigvecs.to(torch.float32)}
    if src_path is not None:
        stats["src_path"] = str(src_path)
    return stats


def _resolve_device(flux: torch.Tensor, device) -> torch.device:
    from ._cabi import VitError

    if flux.is_cuda:
        return flux.device
    if device is None:
        if not torch.cuda.is_available():
            raise VitError("compute_covariance_stats: the accumulation runs on an MI355X and no GPU is visible; there is no "
                           "CPU path (the reference's own compute_covariance_stats is the CPU tool)")
        device = "cuda:0"
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise VitError(f"compute_covariance_stats: device {device} is not a GPU; there is no CPU path for the accumulation")
    return device


def compute_covariance_stats(flux: torch.Tensor, *, chunk_rows: int = 65536, device=None, src_path=None,
                             timings: Optional[dict] = None) -> dict:
    """mean / cov / eigvals / eigvecs of `flux` ([n, L], host or device).  Two passes over chunks of `chunk_rows` rows on the
    GPU (mean, then the centred accumulate), `vit_cov_finish`, then `finish_host`.  A device tensor whose rows the kernels
    can read as they lie (16-byte aligned, L and the row stride multiples of 4) is used in place through its row stride;
    anything else -- a host tensor above all -- goes chunk by chunk through one staging buffer.  `timings` (a dict) receives
    mean_s / accumulate_s / eigh_s."""
    from . import functional as vf

    flux = torch.as_tensor(flux)
    if flux.dim() != 2:
        raise ValueError(f"compute_covariance_stats: flux must be [num_samples, num_features], got {tuple(flux.shape)}")
    n, L = int(flux.shape[0]), int(flux.shape[1])
    if n < 2:
        raise ValueError(f"covariance statistics need at least 2 samples (got {n})")
    if L < 1 or chunk_rows < 1:
        raise ValueError(f"compute_covariance_stats: L={L} chunk_rows={chunk_rows}")
    dev = _resolve_device(flux, device)
    flux = flux.to(torch.float32)  # preprocessor_utils.py:426
    Lp = -(-L // 4) * 4  # vit_colsum reads 4 columns per lane
    in_place = (flux.is_cuda and L == Lp and flux.stride(1) == 1 and flux.stride(0) % 4 == 0 and flux.stride(0) >= L
                and flux.data_ptr() % 16 == 0)
    rows = min(int(chunk_rows), n)
    stage = None if in_place else torch.zeros((rows, Lp), dtype=torch.float32, device=dev)

    def chunks():
        for s in range(0, n, rows):
            e = min(n, s + rows)
            if in_place:
                yield flux[s:e]
            else:
                stage[: e - s, :L].copy_(flux[s:e])
                yield stage[: e - s]

    with torch.cuda.device(dev):
        mean = torch.zeros(Lp, dtype=torch.float32, device=dev)  # columns L .. Lp of the staging buffer are zeros: so are theirs
        t0 = time.perf_counter()
        for i, c in enumerate(chunks()):
            vf.colsum(c, out=mean, accumulate=i > 0)
        vf.cov_mean_finish(mean, n)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        acc = torch.zeros((L, L), dtype=torch.float32, device=dev)
        for c in chunks():
            vf.cov_accumulate(c, mean, acc, cols=L)
        cov = vf.cov_finish(acc, n)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
    if timings is not None:
        timings["mean_s"], timings["accumulate_s"] = t1 - t0, t2 - t1
    return finish_host(mean[:L].cpu(), cov.cpu(), n, src_path=src_path, timings=timings)


def save(stats: dict, path) -> str:
    """Write the statistics where `vit_amd.preprocessor.load_cov_stats` (weights_only=True) reads them: `.npz` by suffix, else
    torch.save; through a temporary file and a rename, so a reader never meets half a file."""
    path = os.path.abspath(str(path))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        if path.endswith(".npz"):
            import numpy as np

            # arrays only: the loader turns every entry into a tensor, so the src_path string stays out of this form
            arrays = {k: v.detach().cpu().numpy() for k, v in stats.items() if isinstance(v, torch.Tensor)}
            with open(tmp, "wb") as f:
                np.savez(f, **arrays)
        else:
            payload = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in stats.items()}
            torch.save(payload, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    from .preprocessor import _COV_CACHE

    _COV_CACHE.pop(path, None)  # a loader that cached an older file of this name must read the new one
    return path


def ensure_cov_file(config: dict, flux_fn, *, world_size: int = 1, chunk_rows: int = 65536, device=None, verbose=True) -> bool:
    """`warmup.cov_compute: true`: when `warmup.cov_path` names a missing file, compute the statistics of `flux_fn()` (the
    training split's flux, called only then) and save them there before the model is built.  Returns whether it did.  Without
    the key nothing happens here, and a missing file raises FileNotFoundError in get_model exactly as before.  More than one
    rank: refused -- this build has no cross-rank handshake on the file."""
    warm = config.get("warmup") or {}
    kind = warm.get("preprocessor")
    path = warm.get("cov_path")
    if not warm.get("cov_compute", False) or kind is None or str(kind).lower() in ("none", "null") or path is None:
        return False
    if os.path.exists(os.path.abspath(str(path))):
        return False
    if int(world_size) > 1:
        raise RuntimeError(f"warmup.cov_compute: {path} does not exist and this run has {world_size} ranks; the statistics are "
                           "computed by one process: run `./launch.sh cov -c CONFIG` first, then start the ranks")
    timings: dict = {}
    flux = flux_fn()
    stats = compute_covariance_stats(flux, chunk_rows=chunk_rows, device=device, timings=timings)
    save(stats, path)
    if verbose:
        print(f"[cov] warmup.cov_compute: wrote {path} (n={flux.shape[0]}, L={flux.shape[1]}; mean {timings['mean_s']:.3f} s, "
              f"accumulate {timings['accumulate_s']:.3f} s, eigh {timings['eigh_s']:.3f} s)")
    return True
