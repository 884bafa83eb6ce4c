"""Covariance statistics on the MI355X (vit_amd/covstats.py over vit_cov_accumulate / vit_cov_finish / vit_colsum): the file
behind `warmup.cov_path`, reference src/prepca/preprocessor_utils.py:399-531.

Truth is float64 on the host from the same f32 input: C64 = c64^T c64 / (n - 1), c64 = X - mean64.  The gate is the worst-case
bound of an f32 FMA chain of n terms, not a tuned number: |C - C64| <= (n + 8) 2^-24 (|c64|^T |c64|) / (n - 1) per entry (n
roundings of the chain, a few more for the centring subtraction, the division and the slice sums).  On the CPU the reference's
own f32 formula and a sequential f32 chain sit at <= 0.14 of that bound on this generator, the uncentred X^T X - n mu mu^T at
>= 600 (offset 100) and the split-bf16 x3 product at 2.8 (n = 37): the bound separates an exact-f32 centred accumulation from
the shortcuts.  Measured on the MI355X: see DESIGN.md section 4."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
CASES = [(37, 100, 0.0), (300, 200, 100.0), (1000, 300, 1000.0), (2500, 520, 100.0)]


@functools.lru_cache(maxsize=None)
def case(n, L, offset):
    """X = (A amp) B + 0.01 noise + offset: 8 components of falling amplitude, float64 normal draws cast to f32; with it the
    float64 truth and the per-entry bound.  Computed once per case and shared; nobody writes into it."""
    g = torch.Generator().manual_seed(1000 * n + L)
    A = torch.randn(n, 8, generator=g, dtype=torch.float64)
    amp = torch.logspace(0, -2, 8, dtype=torch.float64)
    B = torch.randn(8, L, generator=g, dtype=torch.float64)
    noise = torch.randn(n, L, generator=g, dtype=torch.float64)
    X = ((A * amp) @ B + 0.01 * noise + offset).to(torch.float32)
    return (X,) + truth(X)


def truth(X):
    n = X.shape[0]
    X64 = X.double()
    mean64 = X64.mean(0)
    c64 = X64 - mean64
    C64 = c64.t() @ c64 / (n - 1)
    bound = (n + 8) * EPS * (c64.abs().t() @ c64.abs()) / (n - 1)
    return mean64, C64, bound


def worst_ratio(cov, C64, bound):
    return float(((cov.double() - C64).abs() / bound).max())


def check_stats(stats, X, mean64, C64, bound, what):
    n, L = X.shape
    cov, mean = stats["cov"], stats["mean"]
    assert cov.shape == (L, L) and cov.dtype == torch.float32 and mean.shape == (L,) and int(stats["num_samples"]) == n
    ratio = worst_ratio(cov, C64, bound)
    mean_ratio = float(((mean.double() - mean64).abs() / (n * EPS * X.double().abs().mean(0))).max())
    print(f"[cov {what} n={n} L={L}] worst |C - C64| / bound = {ratio:.3f}; worst mean error / bound = {mean_ratio:.3f}")
    assert torch.equal(cov, cov.t()), "cov must be bitwise symmetric"
    assert ratio <= 1.0, f"{what}: covariance outside the f32 FMA-chain bound ({ratio:.3f} x)"
    assert mean_ratio <= 1.0, f"{what}: mean outside n 2^-24 mean|x| ({mean_ratio:.3f} x)"


@pytest.mark.parametrize("n,L,offset", CASES)
def test_covariance_within_f32_chain_bound(dev, n, L, offset):
    from vit_amd import covstats

    X, mean64, C64, bound = case(n, L, offset)
    stats = covstats.compute_covariance_stats(X.to(dev))  # device-resident, read in place
    check_stats(stats, X, mean64, C64, bound, "device")
    again = covstats.compute_covariance_stats(X.to(dev))
    assert torch.equal(stats["cov"], again["cov"]) and torch.equal(stats["mean"], again["mean"]), "two runs must agree bit for bit"
    host = covstats.compute_covariance_stats(X, device=dev)  # host tensor: staged chunk by chunk
    check_stats(host, X, mean64, C64, bound, "host")
    if (n, L) == (300, 200):  # the same rows inside a wider buffer: ldx = L + 8, the columns beside them must not be read
        wide = torch.full((n, L + 8), 1e6, dtype=torch.float32, device=dev)
        wide[:, :L] = X.to(dev)
        view = wide[:, :L]
        assert view.stride(0) == L + 8
        strided = covstats.compute_covariance_stats(view)
        check_stats(strided, X, mean64, C64, bound, "ldx = L + 8")
        assert torch.equal(strided["cov"], stats["cov"])  # same values, same plan: same bits
    if (n, L) == (1000, 300):  # chunks of 400 / 400 / 200 rows: within the bound too (the bits may differ from one call's)
        chunked = covstats.compute_covariance_stats(X.to(dev), chunk_rows=400)
        check_stats(chunked, X, mean64, C64, bound, "chunk_rows=400")
        chunked_host = covstats.compute_covariance_stats(X, chunk_rows=400, device=dev)
        check_stats(chunked_host, X, mean64, C64, bound, "host chunk_rows=400")


def test_odd_width_and_unaligned_rows(dev):
    """L = 131 (no multiple of 4, two tiles, the second 3 columns wide): compute_covariance_stats stages it into padded rows;
    the kernel itself also takes the unpadded rows (stride 131, rows not 16-byte aligned: the scalar loads) and a single row."""
    from vit_amd import covstats
    from vit_amd import functional as vf

    n, L = 70, 131
    X, mean64, C64, bound = case(n, L, 10.0)
    stats = covstats.compute_covariance_stats(X.to(dev))
    check_stats(stats, X, mean64, C64, bound, "odd L")
    xd = X.to(dev)
    assert xd.stride(0) == L
    mean = stats["mean"].to(dev)
    acc = torch.zeros(L, L, device=dev)
    vf.cov_accumulate(xd[:1], mean, acc)      # n = 1
    vf.cov_accumulate(xd[1:], mean, acc)      # base address 4-byte aligned only
    cov = vf.cov_finish(acc, n).cpu()
    ratio = worst_ratio(cov, C64, bound)
    print(f"[cov unaligned n={n} L={L}] worst |C - C64| / bound = {ratio:.3f}")
    assert torch.equal(cov, cov.t()) and ratio <= 1.0


def test_eigenvalues_weyl(dev):
    """Weyl: max |lambda - lambda64| <= ||C - C64||_2 <= ||bound||_F, plus the f32 eigensolver's own 16 L 2^-24 lambda_0."""
    from vit_amd import covstats

    X, mean64, C64, bound = case(300, 200, 100.0)
    stats = covstats.compute_covariance_stats(X.to(dev))
    lam64 = torch.linalg.eigvalsh(C64).flip(0)
    lam = stats["eigvals"].double()
    gate = float(bound.norm()) + 16 * 200 * EPS * float(lam64[0])
    err = float((lam - lam64).abs().max())
    print(f"[cov eig] max |lambda - lambda64| = {err:.3e} ({err / float(lam64[0]):.2e} lambda_0), gate {gate:.3e}")
    assert err <= gate
    assert bool((lam[:-1] >= lam[1:]).all()) and float(lam.min()) >= 0.0
    V = stats["eigvecs"].double()
    assert float((V.t() @ V - torch.eye(200, dtype=torch.float64)).abs().max()) <= 16 * 200 * EPS


def test_fixture_agrees_with_reference(dev):
    """tests/golden/cov.npz: the reference's own compute_covariance_stats on a [64, 48] input (tools/make_cov_golden.py).  Both
    sides are f32 accumulations of the same 64 terms: they agree within the sum of both bounds."""
    from vit_amd import covstats

    g = np.load(os.path.join(ROOT, "tests", "golden", "cov.npz"))
    X = torch.from_numpy(g["x"])
    mean64, C64, bound = truth(X)
    stats = covstats.compute_covariance_stats(X, device=dev)
    check_stats(stats, X, mean64, C64, bound, "fixture")
    ref_cov, ref_mean = torch.from_numpy(g["cov"]), torch.from_numpy(g["mean"])
    ratio = float(((stats["cov"].double() - ref_cov.double()).abs() / (2 * bound)).max())
    ref_ratio = worst_ratio(ref_cov, C64, bound)
    print(f"[cov fixture] |ours - reference| / (2 bound) = {ratio:.3f}; reference vs float64 / bound = {ref_ratio:.3f}")
    assert ratio <= 1.0
    assert float((stats["mean"].double() - ref_mean.double()).abs().max()) <= 2 * 64 * EPS * float(X.abs().mean(0).max())
    lam_ref = torch.from_numpy(g["eigvals"]).double()
    assert float((stats["eigvals"].double() - lam_ref).abs().max()) <= 2 * float(bound.norm()) + 16 * 48 * EPS * float(lam_ref[0])
    assert int(stats["num_samples"]) == int(g["num_samples"])


def test_downstream_zca_matrix(dev):
    """What the statistics are for: the ZCA matrix (eps 1e-5, shrinkage 0.1) from the GPU statistics against the one from
    float64 statistics.  Yardstick: the same distance for statistics computed by the reference's f32 formula with torch on the
    CPU, here in the test -- never this build's own output.  Gate: 4 x that distance (a blocked CPU matmul and a k-ordered
    chain differ by summation order: <= 5.3 x on the covariance itself at n = 2500, less at n = 300)."""
    from vit_amd import covstats
    from vit_amd.preprocessor import compute_zca_matrix

    X, mean64, C64, bound = case(300, 200, 100.0)
    n = X.shape[0]

    def sorted_eigh(cov):  # _sorted_eigh_sym, preprocessor_utils.py:44-62
        lam, vec = torch.linalg.eigh(0.5 * (cov + cov.t()))
        lam = torch.clamp(lam, min=0.0)
        idx = torch.argsort(lam, descending=True)
        return lam[idx], vec[:, idx]

    lam64, vec64 = sorted_eigh(C64)
    Z64 = compute_zca_matrix(vec64, lam64, eps=1e-5, shrinkage=0.1)
    centred = X - X.mean(dim=0)                      # the reference's f32 formula, :427-429
    lam_r, vec_r = sorted_eigh(centred.t().matmul(centred) / (n - 1))
    Zr = compute_zca_matrix(vec_r, lam_r, eps=1e-5, shrinkage=0.1)
    stats = covstats.compute_covariance_stats(X.to(dev))
    Zg = compute_zca_matrix(stats["eigvecs"], stats["eigvals"], eps=1e-5, shrinkage=0.1)
    d_ref = float((Zr.double() - Z64).norm() / Z64.norm())
    d_gpu = float((Zg.double() - Z64).norm() / Z64.norm())
    print(f"[cov zca] ||Z - Z64|| / ||Z64||: GPU statistics {d_gpu:.3e}, reference f32 formula on the CPU {d_ref:.3e}, "
          f"ratio {d_gpu / d_ref:.2f} (gate 4)")
    assert d_gpu <= 4.0 * d_ref


def test_errors(dev):
    from vit_amd import covstats

    with pytest.raises(ValueError):
        covstats.compute_covariance_stats(torch.zeros(1, 16, device=dev))
    with pytest.raises(ValueError):
        covstats.compute_covariance_stats(torch.zeros(16, device=dev))


def test_cli_cov_then_zca_fit_and_cov_compute(dev, tmp_path):
    """`launch.sh cov --synthetic 512` on a C1-sized config (L = 4096, three chunks of 200 rows) writes the statistics; one
    `Trainer.fit` epoch with `warmup: {preprocessor: zca, r: 64, cov_path: <that file>}` ends with a finite loss; the same
    configuration with `cov_compute: true` and no file computes the file on the way and builds the same front bit for bit."""
    import yaml

    from scripts import run as run_script
    from vit_amd.preprocessor import load_cov_stats
    from vit_amd.trainer import Trainer

    def config(cov_path, **warm):
        return {
            "project": "t",
            "model": dict(name="vit", task_type="reg", image_size=4096, patch_size=32, hidden_size=32, num_hidden_layers=3,
                          num_attention_heads=2, stride_size=32, proj_fn="SW"),
            "train": dict(batch_size=64, ep=1, precision="32"),
            "loss": {"name": "mae"}, "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"},
            "noise": {"noise_level": 0},
            "warmup": dict(preprocessor="zca", r=64, cov_path=str(cov_path), freeze_epochs=-1, cov_chunk_rows=200, **warm),
        }

    def build(cfg, name):
        path = tmp_path / name
        path.write_text(yaml.safe_dump(cfg))
        args = types.SimpleNamespace(config=str(path), gpu=1, debug=0, seed=42, synthetic=512, save=False, ckpt=None)
        return args, run_script.build(args)

    f1, f2 = tmp_path / "stats" / "cov.pt", tmp_path / "stats2" / "cov.pt"
    cpath = tmp_path / "c.yaml"
    cpath.write_text(yaml.safe_dump(config(f1)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run(["bash", os.path.join(ROOT, "launch.sh"), "cov", "-c", str(cpath), "--synthetic", "512"],
                       capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "n=512 L=4096" in r.stdout and "leading eigenvalues" in r.stdout and "trailing eigenvalues" in r.stdout
    stats = load_cov_stats(str(f1))  # weights_only=True
    assert stats["cov"].shape == (4096, 4096) and int(stats["num_samples"]) == 512 and torch.equal(stats["cov"], stats["cov"].t())
    assert bool((stats["eigvals"][511:] == 0).all()) and float(stats["eigvals"][0]) > 0

    args, (cfg, module, data) = build(config(f1), "run1.yaml")
    assert module.model.name.startswith("ZCA64_fzperm")
    w1 = module.model.preprocessor.linear.weight.detach().cpu().clone()
    b1 = module.model.preprocessor.linear.bias.detach().cpu().clone()
    trainer = Trainer(cfg["train"], device=dev, verbose=False)
    train_loader, val_loader = data.fit_loaders(args.debug)
    hist = trainer.fit(module, train_loader, val_loader)
    logged = {k: float(v) for k, v in hist[-1].items() if "loss" in k}
    print(f"[cov e2e] epoch metrics: {logged}")
    assert logged and all(np.isfinite(v) for v in logged.values())

    assert not f2.exists()
    _, (_, module2, _) = build(config(f2, cov_compute=True), "run2.yaml")
    assert f2.exists()
    w2 = module2.model.preprocessor.linear.weight.detach().cpu()
    b2 = module2.model.preprocessor.linear.bias.detach().cpu()
    assert torch.equal(load_cov_stats(str(f2))["cov"], stats["cov"])
    assert torch.equal(w1, w2) and torch.equal(b1, b2)
