"""Host side of the covariance statistics (vit_amd/covstats.py, scripts/cov.py, `warmup.cov_compute`): everything that needs no
GPU.  Reference: src/prepca/preprocessor_utils.py:44-62 (_sorted_eigh_sym), :399-531 (compute / load-or-compute).
tests/golden/cov.npz holds the reference's own mean / cov / eigvals for a [64, 48] input (tools/make_cov_golden.py)."""
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "cov.npz"))
    return {k: torch.from_numpy(np.asarray(g[k])) for k in g.files}


def test_finish_host_reproduces_reference_eigenvalues():
    from vit_amd import covstats

    g = fixture()
    L, n = 48, int(g["num_samples"])
    assert tuple(g["x"].shape) == (64, L) and n == 64
    stats = covstats.finish_host(g["mean"], g["cov"], n)
    assert set(stats) == {"mean", "cov", "num_samples", "eigvals", "eigvecs"}
    assert stats["mean"].shape == (L,) and stats["cov"].shape == (L, L) and stats["eigvals"].shape == (L,)
    assert stats["eigvecs"].shape == (L, L)
    assert all(stats[k].dtype == torch.float32 for k in ("mean", "cov", "eigvals", "eigvecs"))
    assert stats["num_samples"].dim() == 0 and not stats["num_samples"].is_floating_point() and int(stats["num_samples"]) == n
    lam, V = stats["eigvals"], stats["eigvecs"]
    lam0 = float(g["eigvals"][0])
    gate = 16 * L * EPS * lam0
    err = float((lam - g["eigvals"]).abs().max())
    rec = float(((V * lam) @ V.t() - g["cov"]).abs().max())
    print(f"[finish_host] max |lambda - reference| = {err:.3e}, max |V diag(lambda) V^T - cov| = {rec:.3e}, gate {gate:.3e}")
    assert err <= gate
    assert bool((lam[:-1] >= lam[1:]).all()) and float(lam.min()) >= 0.0
    assert rec <= gate
    assert torch.equal(stats["cov"], stats["cov"].t()) and torch.equal(stats["mean"], g["mean"])
    with_src = covstats.finish_host(g["mean"], g["cov"], n, src_path="/data/train.npz")
    assert with_src["src_path"] == "/data/train.npz"
    with pytest.raises(ValueError):
        covstats.finish_host(g["mean"], g["cov"], 1)


def test_rank_deficient_input_has_exactly_zero_tail():
    """20 samples of 48 features: rank <= 19, so the eigenvalues from position 19 on are exactly 0, the 19 before positive."""
    from vit_amd import covstats

    n, L = 20, 48
    X = torch.randn(n, L, generator=torch.Generator().manual_seed(7)) + 3.0
    mean = X.mean(dim=0)
    c = X - mean
    stats = covstats.finish_host(mean, c.t().matmul(c) / (n - 1), n)
    lam = stats["eigvals"]
    assert bool((lam[n - 1:] == 0).all())
    assert bool((lam[: n - 1] > 1e-3 * lam[0]).all()) and bool((lam[:-1] >= lam[1:]).all())
    V = stats["eigvecs"]
    assert float((V.t() @ V - torch.eye(L)).abs().max()) <= 16 * L * EPS


@pytest.mark.parametrize("suffix", [".pt", ".npz"])
def test_save_roundtrip_and_fronts(tmp_path, suffix):
    from vit_amd import covstats
    from vit_amd.builder import get_model
    from vit_amd.preprocessor import load_cov_stats

    g = fixture()
    stats = covstats.finish_host(g["mean"], g["cov"], 64, src_path="train.npz")
    path = tmp_path / "deep" / "dir" / f"cov{suffix}"
    assert covstats.save(stats, path) == str(path)
    assert sorted(os.listdir(path.parent)) == [f"cov{suffix}"]  # the temporary file is gone
    back = load_cov_stats(str(path))  # .pt: torch.load(weights_only=True)
    for k in ("mean", "cov", "eigvals", "eigvecs"):
        assert torch.equal(back[k], stats[k]) and back[k].dtype == torch.float32, k
    assert int(back["num_samples"]) == 64
    # saving again under the same name must not leave the loader on its cached copy
    stats2 = dict(stats, mean=stats["mean"] + 1.0)
    covstats.save(stats2, path)
    assert torch.equal(load_cov_stats(str(path))["mean"], stats2["mean"])
    covstats.save(stats, path)

    def cfg(**warm):
        return {"model": dict(name="vit", task_type="reg", image_size=48, patch_size=8, hidden_size=32, num_hidden_layers=1,
                              num_attention_heads=2, stride_size=8, proj_fn="SW"),
                "loss": {"name": "mae"}, "warmup": dict(cov_path=str(path), **warm)}

    zca = get_model(cfg(preprocessor="zca", shrinkage=0.1))
    assert zca.preprocessor.linear.weight.shape == (48, 48) and zca.name.startswith("ZCA_fz0_s1")
    pca = get_model(cfg(preprocessor="pca", r=16))
    assert pca.preprocessor.linear.weight.shape == (16, 48) and pca.config.image_size == 16
    assert torch.equal(pca.preprocessor.linear.weight, stats["eigvecs"][:, :16].t())
    assert torch.allclose(pca.preprocessor.linear.bias, -(stats["mean"] @ stats["eigvecs"][:, :16]))
    att = get_model(cfg(preprocessor="attention", r=16))
    assert att.preprocessor.q_lin.weight.shape == (16, 48)


def test_cov_script_arguments():
    from scripts import cov

    a = cov.parse_args(["-f", "c.yaml", "--out", "o.pt", "--synthetic", "512", "--limit", "100", "--chunk-rows", "200"])
    assert (a.config, a.out, a.synthetic, a.limit, a.chunk_rows) == ("c.yaml", "o.pt", 512, 100, 200)
    d = cov.parse_args([])
    assert (d.config, d.out, d.synthetic, d.limit, d.chunk_rows) == ("configs/baseline.yaml", None, None, None, None)
    assert cov.chunk_rows_of({}, None) == 65536 and cov.chunk_rows_of({"warmup": {"cov_chunk_rows": 200}}) == 200
    assert cov.chunk_rows_of({"warmup": {"cov_chunk_rows": 200}}, 50) == 50
    # --synthetic N: the flux `launch.sh run --synthetic N` trains on (seed 1), --limit cuts it
    from scripts.run import SyntheticSpectra

    config = {"model": {"image_size": 96, "task_type": "reg"}}
    flux = cov.training_flux(config, synthetic=12, limit=10)
    assert torch.equal(flux, SyntheticSpectra(12, 96, "reg", 3, 1, stage="train").flux[:10])
    assert "scripts/cov.py" in open(os.path.join(ROOT, "launch.sh")).read()
    import subprocess

    for mode in ("lr", "sweep"):  # still refused, before any Python starts
        r = subprocess.run(["bash", os.path.join(ROOT, "launch.sh"), mode], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "outside the MI355X hot path" in r.stdout


def _write_config(tmp_path, **warm):
    import yaml

    cfg = {"model": dict(name="vit", task_type="reg", image_size=48, patch_size=8, hidden_size=32, num_hidden_layers=1,
                         num_attention_heads=2, stride_size=8, proj_fn="SW"),
           "train": dict(batch_size=4, ep=1, precision="32"), "loss": {"name": "mae"}, "opt": {"type": "AdamW", "lr": 1e-3},
           "data": {"param": "log_g"}, "noise": {"noise_level": 0},
           "warmup": dict(preprocessor="zca", cov_path=str(tmp_path / "missing" / "cov.pt"), **warm)}
    path = tmp_path / "c.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return cfg, types.SimpleNamespace(config=str(path), gpu=1, debug=0, seed=42, synthetic=16, save=False, ckpt=None)


def test_missing_file_without_cov_compute_still_raises(tmp_path):
    from scripts import run as run_script
    from vit_amd import covstats
    from vit_amd.builder import get_model

    cfg, args = _write_config(tmp_path)
    called = []
    assert covstats.ensure_cov_file(cfg, lambda: called.append(1)) is False and not called  # default off: nothing happens here
    with pytest.raises(FileNotFoundError):
        get_model(cfg)
    with pytest.raises(FileNotFoundError):
        run_script.build(args)
    cfg["warmup"]["cov_compute"] = False
    with pytest.raises(FileNotFoundError):
        get_model(cfg)
    assert not os.path.exists(tmp_path / "missing")


def test_cov_compute_refuses_more_than_one_rank(tmp_path, monkeypatch):
    from scripts import run as run_script
    from vit_amd import covstats

    cfg, args = _write_config(tmp_path, cov_compute=True)
    called = []
    with pytest.raises(RuntimeError, match=r"launch\.sh cov"):
        covstats.ensure_cov_file(cfg, lambda: called.append(1), world_size=2)
    assert not called  # refused before any data is read
    args.gpu = 2
    with pytest.raises(RuntimeError, match=r"launch\.sh cov"):
        run_script.build(args)
    args.gpu = 1
    monkeypatch.setenv("WORLD_SIZE", "4")
    with pytest.raises(RuntimeError, match=r"launch\.sh cov"):
        run_script.ensure_cov_stats(args, cfg)
    # an existing file: nothing to do, whatever the rank count
    os.makedirs(tmp_path / "missing")
    (tmp_path / "missing" / "cov.pt").write_bytes(b"x")
    assert covstats.ensure_cov_file(cfg, lambda: called.append(1), world_size=2) is False and not called


def test_cpu_tensor_without_gpu_is_an_error(monkeypatch):
    from vit_amd import covstats
    from vit_amd._cabi import VitError

    with pytest.raises(ValueError):
        covstats.compute_covariance_stats(torch.zeros(1, 8))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(VitError, match="no CPU path"):
        covstats.compute_covariance_stats(torch.zeros(4, 8))
    with pytest.raises(VitError, match="no CPU path"):
        covstats.compute_covariance_stats(torch.zeros(4, 8), device="cpu")
