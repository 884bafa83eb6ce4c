#!/usr/bin/env python3
"""Generate tests/golden/cov.npz: a small seeded input and the REFERENCE's own covariance statistics for it.

    python tools/make_cov_golden.py --reference /path/to/ViskaWei-VIT [--out tests/golden/cov.npz]

Imports the reference's src.prepca.preprocessor_utils.compute_covariance_stats at run time (the absent h5py / lightning
packages are stubbed for the import only, by oracle.make_golden's helper; MPLBACKEND=Agg because the module pulls
matplotlib in).  The fixture holds data only -- the input `x` [64, 48] f32 (seed 20240607, offset +5) and the reference's
`mean`, `cov`, `eigvals`, `num_samples` -- nothing of the reference's program text.  Tests read the fixture, never the
reference tree."""
import argparse
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, L, SEED, OFFSET = 64, 48, 20240607, 5.0


def make_input() -> torch.Tensor:
    """Spectra-like rows: 6 shared components of falling amplitude + white noise + a common offset (f64 draws, cast to f32)."""
    g = torch.Generator().manual_seed(SEED)
    a = torch.randn(N, 6, generator=g, dtype=torch.float64) * torch.logspace(0, -2, 6, dtype=torch.float64)
    b = torch.randn(6, L, generator=g, dtype=torch.float64)
    noise = torch.randn(N, L, generator=g, dtype=torch.float64)
    return (a @ b + 0.01 * noise + OFFSET).to(torch.float32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reference", default=os.environ.get("VIT_REFERENCE"), help="root of a checkout of the reference project")
    p.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cov.npz"))
    args = p.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        raise SystemExit("pass --reference DIR (or set VIT_REFERENCE): the checkout whose compute_covariance_stats makes the fixture")
    from oracle import make_golden as mg

    mg.REF = args.reference
    mg._import_reference()
    from src.prepca.preprocessor_utils import compute_covariance_stats

    x = make_input()
    stats = compute_covariance_stats(x.clone(), save_path=None)
    lam = stats.eigvals
    assert stats.cov.shape == (L, L) and torch.equal(stats.cov, stats.cov.t()) and bool((lam[:-1] >= lam[1:]).all())
    np.savez(args.out, x=x.numpy(), mean=stats.mean.numpy(), cov=stats.cov.numpy(), eigvals=lam.numpy(),
             num_samples=np.int64(stats.num_samples))
    print(f"wrote {args.out}: x {tuple(x.shape)}, lambda_0 {float(lam[0]):.6g}, lambda_min {float(lam[-1]):.3g}, "
          f"{os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
