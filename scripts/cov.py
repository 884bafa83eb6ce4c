#!/usr/bin/env python3
"""`launch.sh cov`: compute the covariance statistics file that `warmup.preprocessor: zca | pca | attention` reads
(`warmup.cov_path`) from the config's training split -- the reference's compute_covariance_stats /
load_or_compute_covariance (src/prepca/preprocessor_utils.py:399-531) with the O(n L^2) part on the MI355X
(vit_amd/covstats.py) and the eigendecomposition on the host.

    ./launch.sh cov -c CONFIG [--out PATH] [--synthetic N] [--limit N] [--chunk-rows R]

The spectra are the `flux` the training `SpecDataset` holds, i.e. what the preprocessor will be fed (zero clip included);
`--synthetic N` takes the N seeded spectra a `launch.sh run --synthetic N` trains on.  The file goes to `--out`, else to the
config's `warmup.cov_path`."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="covariance statistics of the training split (MI355X path)")
    p.add_argument("-f", "--config", type=str, default="configs/baseline.yaml")
    p.add_argument("--out", type=str, default=None, help="output file (.pt, or .npz by suffix); default: the config's warmup.cov_path")
    p.add_argument("--synthetic", type=int, default=None,
                   help="use the N seeded synthetic spectra of `launch.sh run --synthetic N` instead of data.file_path")
    p.add_argument("--limit", type=int, default=None, help="use only the first N spectra of the split")
    p.add_argument("--chunk-rows", type=int, default=None,
                   help="rows per GPU pass (default: warmup.cov_chunk_rows of the config, else 65536)")
    p.add_argument("-g", "--gpu", type=int, default=None, help="accepted for launch.sh compatibility; one GPU computes the file")
    return p.parse_args(argv)


def training_flux(config, synthetic=None, limit=None):
    """[n, L] f32 on the host: the flux of the training split as the model's front will see it."""
    if synthetic is not None:
        from scripts.run import SyntheticSpectra

        m = config["model"]
        # seed 1, stage 'train': DataSource.fit_loaders' training set; the labels' shape does not touch the flux
        flux = SyntheticSpectra(int(synthetic), m["image_size"], m.get("task_type", "reg"), 1, 1, stage="train").flux
    else:
        from vit_amd.data import SpecDataModule

        dm = SpecDataModule.from_config(config)
        if not dm.paths["train"]:
            raise SystemExit("the config names no training file (data.file_path); pass --synthetic N for seeded synthetic spectra")
        flux = dm._load("train", None).flux
    return flux if limit is None else flux[: int(limit)]


def chunk_rows_of(config, override=None) -> int:
    return int(override if override is not None else (config.get("warmup") or {}).get("cov_chunk_rows", 65536))


def main(args):
    from vit_amd import covstats
    from vit_amd.utils import load_config

    config = load_config(args.config)
    out = args.out or (config.get("warmup") or {}).get("cov_path")
    if not out:
        raise SystemExit("nowhere to write: pass --out PATH or set warmup.cov_path in the config")
    t0 = time.perf_counter()
    flux = training_flux(config, args.synthetic, args.limit)
    t_load = time.perf_counter() - t0
    src = f"synthetic:{args.synthetic}" if args.synthetic is not None else (config.get("data") or {}).get("file_path")
    timings = {}
    stats = covstats.compute_covariance_stats(flux, chunk_rows=chunk_rows_of(config, args.chunk_rows), src_path=src, timings=timings)
    path = covstats.save(stats, out)
    n, L = flux.shape
    lam = stats["eigvals"]
    fmt = lambda v: " ".join(f"{float(x):.6g}" for x in v)  # noqa: E731
    print(f"[cov] n={n} L={L} source={src} (loaded in {t_load:.2f} s)")
    print(f"[cov] GPU pass 1 (mean) {timings['mean_s'] * 1e3:.1f} ms, pass 2 (centred accumulate + finish) "
          f"{timings['accumulate_s'] * 1e3:.1f} ms, host eigh {timings['eigh_s']:.2f} s")
    print(f"[cov] leading eigenvalues:  {fmt(lam[:5])}")
    print(f"[cov] trailing eigenvalues: {fmt(lam[-5:])}")
    print(f"[cov] wrote {path}")
    return path


if __name__ == "__main__":
    main(parse_args())
