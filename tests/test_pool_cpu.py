"""Global average pooling (`model.global_pool: avg`, include/vit_amd_pool.h) without a GPU: config validation, that the default
config and the parameter layout did not move, the run-name suffix, the host restatement of the kernels (tests/_pool_ref.py)
against a float64 mean and against autograd, and the C ABI's declarations."""
import copy
import json
import os
import types

import numpy as np
import pytest
import torch

import _pool_ref as pr

KW = dict(image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, stride_size=32)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def yaml_like(**model):
    return {"model": dict(dict(task_type="cls", num_labels=3, proj_fn="SW", **KW), **model), "data": {"param": "log_g"}}


def test_config_accepts_token_and_avg_and_rejects_the_rest():
    from vit_amd.config import ViTConfig, get_vit_config

    assert ViTConfig(task_type="reg", **KW).global_pool == "token"
    assert get_vit_config(yaml_like()).global_pool == "token"
    for pool in ("token", "avg"):
        assert ViTConfig(task_type="cls", global_pool=pool, **KW).global_pool == pool
        assert get_vit_config(yaml_like(global_pool=pool)).global_pool == pool
        assert get_vit_config(yaml_like(global_pool=pool, task_type="reg")).global_pool == pool
    for bad in ("max", "AVG", "", None, 1, True, ["avg"]):
        with pytest.raises(ValueError, match="global_pool"):
            ViTConfig(task_type="cls", global_pool=bad, **KW)
        with pytest.raises(ValueError, match="global_pool"):
            get_vit_config(yaml_like(global_pool=bad))
    with pytest.raises(ValueError, match="global_pool.*mim|mim.*global_pool"):
        ViTConfig(task_type="mim", global_pool="avg", **KW)
    with pytest.raises(ValueError, match="global_pool"):
        get_vit_config(dict(yaml_like(global_pool="avg", task_type="mim"), mim={"mask_ratio": 0.5}))
    assert ViTConfig(task_type="mim", **KW).global_pool == "token"


def test_default_config_is_the_golden_one():
    """tests/golden/config.json (the reference's own get_vit_config): every pinned field as before, and the pooling those
    configs get is the reference's CLS row."""
    from vit_amd.config import get_vit_config

    with open(os.path.join(GOLDEN, "config.json")) as f:
        doc = json.load(f)
    assert doc["cases"]
    for name, cfg in doc["cases"].items():
        c = copy.deepcopy(cfg)
        vc = get_vit_config(c)
        assert vc.global_pool == "token", name
        for k, v in doc["expected"][name]["fields"].items():
            assert getattr(vc, k) == v or (v is None and getattr(vc, k) is None), (name, k)
        assert "global_pool" not in c["model"]


def test_layout_buckets_and_state_order_do_not_depend_on_the_pooling():
    from vit_amd.config import ViTConfig
    from vit_amd.engine import ParamLayout

    for task, pos, nl in (("reg", None, 1), ("cls", "learned", 5), ("cls", "rope", 3)):
        a = ParamLayout(ViTConfig(task_type=task, pos_encoding_type=pos, num_labels=nl, **KW))
        b = ParamLayout(ViTConfig(task_type=task, pos_encoding_type=pos, num_labels=nl, global_pool="avg", **KW))
        assert a.entries == b.entries and a.state_order == b.state_order and a.buckets() == b.buckets()
        assert (a.n_trainable, a.n_total, a.head) == (b.n_trainable, b.n_total, b.head)


def test_run_name_gains_gap_under_avg_only():
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT, build_model_name

    with open(os.path.join(GOLDEN, "names.json")) as f:
        doc = json.load(f)
    for rec in doc["names"]:
        c = rec["case"]
        full = {"noise": {"noise_level": c["noise"]}}
        ns = types.SimpleNamespace(**{k: v for k, v in c.items() if k != "noise"})
        assert build_model_name(ns, "ViT", full_config=full) == rec["ViT"]  # no global_pool attribute at all
        ns.global_pool = "token"
        assert build_model_name(ns, "ViT", full_config=full) == rec["ViT"]
        ns.global_pool = "avg"
        assert build_model_name(ns, "ViT", full_config=full) == rec["ViT"] + "_gap"
        assert build_model_name(ns, "ZCA_ViT") == rec["plain"] + "_gap"
    token = MyViT(ViTConfig(task_type="cls", num_labels=3, **KW))
    avg = MyViT(ViTConfig(task_type="cls", num_labels=3, global_pool="avg", **KW))
    assert avg.name == token.name + "_gap" and not token.name.endswith("_gap")
    assert list(avg.state_dict()) == list(token.state_dict())
    assert avg.engine.avg_pool and not token.engine.avg_pool
    # the switch `launch.sh test --ckpt` uses: the same tensors, the other arithmetic, the other name
    token.set_global_pool("avg")
    assert token.engine.avg_pool and token.config.global_pool == "avg" and token.name == avg.name
    token.set_global_pool("token")
    assert not token.engine.avg_pool and not token.name.endswith("_gap")
    with pytest.raises(ValueError, match="global_pool"):
        token.set_global_pool("max")


def test_checkpoint_config_carries_the_pooling_mode():
    from vit_amd.trainer import saved_global_pool

    assert saved_global_pool({"state_dict": {}}) is None
    assert saved_global_pool({"hyper_parameters": {"config": {"model": {"hidden_size": 8}}}}) == "token"
    assert saved_global_pool({"hyper_parameters": {"config": yaml_like(global_pool="avg")}}) == "avg"


@pytest.mark.parametrize("offset", [0.0, 1e4])
@pytest.mark.parametrize("shape", pr.SHAPES)
def test_restated_forward_is_within_the_f32_bound_of_a_float64_mean(shape, offset):
    B, T, D, first = shape
    x = pr.kernel_input(shape, 1000 + T + D, offset)
    got = pr.pool_fwd(x, first)
    assert got.dtype == np.float32 and got.shape == (B, D)
    ref = x[:, first:, :].astype(np.float64).mean(axis=1)
    err, lim = np.abs(got.astype(np.float64) - ref), pr.bound(x, first)
    print(f"[pool restatement {shape} offset {offset:g}] worst error / bound {float((err / lim).max()):.3f}")
    assert bool((err <= lim).all())
    if T - first == 1:  # one row: the row itself, bit for bit
        assert np.array_equal(got, x[:, first, :])


def test_restated_order_is_the_documented_one():
    """Eleven rows behind first = 1: partial 0 takes rows 1 and 9, partial 1 rows 2 and 10, partial 2 rows 3 and 11, the rest
    one row each; then the partials in ascending order -- written out by hand."""
    f = np.float32
    x = pr.kernel_input((1, 12, 3, 1), 7, 100.0)
    r = [x[0, t] for t in range(12)]
    s = f(r[1] + r[9])
    s = f(s + f(r[2] + r[10]))
    s = f(s + f(r[3] + r[11]))
    for t in range(4, 9):
        s = f(s + r[t])
    assert np.array_equal(pr.pool_fwd(x, 1)[0], f(s * f(1.0 / 11)))
    assert pr.inv_count(12, 1) == np.float32(1 / 11)


@pytest.mark.parametrize("shape", pr.SHAPES)
def test_restated_backward_is_the_adjoint(shape):
    B, T, D, first = shape
    rng = np.random.default_rng(5)
    x, g = rng.standard_normal((B, T, D)).astype(np.float32), rng.standard_normal((B, D)).astype(np.float32)
    dx = pr.pool_bwd(g, T, first)
    assert dx.shape == (B, T, D) and not dx[:, :first].any()
    assert np.array_equal(dx[:, first:], np.broadcast_to((g * np.float32(1 / (T - first)))[:, None, :], (B, T - first, D)))
    lhs = float((pr.pool_fwd(x, first).astype(np.float64) * g).sum())
    rhs = float((x.astype(np.float64) * dx).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs), 1e-3)


def test_oracle_step_gradient_of_last_hidden_state_is_the_restated_backward():
    from oracle import refvit

    rc = refvit.RefConfig(task_type="cls", num_labels=3, pos_encoding_type="learned", **KW)
    sd = refvit.make_state_dict(rc, 3)
    flux, _, labels = refvit.make_inputs(rc, 4, 4)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    loss, logits, out = pr.oracle_step(rc, params, flux, labels, False, None, keep_last_grad=True)
    assert logits.shape == (4, 3) and out.last_hidden_state.shape == (4, rc.num_patches + 1, rc.hidden_size)
    # dpooled by hand: the head is one Linear, the loss is refvit's cross entropy
    pooled = out.last_hidden_state.detach()[:, 1:].mean(1).requires_grad_(True)
    refvit.loss_fn(rc, torch.nn.functional.linear(pooled, sd["classifier.weight"], sd["classifier.bias"]), labels).backward()
    loss.backward()
    got = out.last_hidden_state.grad.numpy()
    want = pr.pool_bwd(pooled.grad.numpy(), rc.num_patches + 1, 1)
    assert not got[:, 0].any() and float(np.abs(want).max()) > 0
    assert float(np.abs(got - want).max()) <= 1e-6 * float(np.abs(want).max())
    assert float(params["vit.embeddings.cls_token"].grad.abs().max()) > 0  # CLS still feeds the attention of L > 0 layers
    # the pooled logits are not the CLS head's
    cls_logits = refvit.forward(rc, sd, flux, labels).logits
    assert float((logits.detach() - cls_logits).abs().max()) > 1e-3
    # soft targets: torch's cross entropy with probabilities
    t = torch.softmax(torch.randn(4, 3, generator=torch.Generator().manual_seed(1)), -1)
    soft, lg, _ = pr.oracle_step(rc, sd, flux, t, False, None, soft="ce")
    assert abs(float(soft) - float(-(t * torch.log_softmax(lg, -1)).sum(1).mean())) < 1e-6


def test_header_declares_the_two_exports_and_the_binding_knows_them():
    from vit_amd import _cabi
    from vit_amd.build import HEADERS, SOURCES

    names = _cabi.declared_symbols()
    for n in ("vit_token_pool_fwd", "vit_token_pool_bwd"):
        assert n in names and len(_cabi._PROTOS[n]) == 8
    assert "pool.hip" in SOURCES and any(h.endswith("vit_amd_pool.h") for h in HEADERS)
    text = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "vit_amd_pool.h")).read()
    assert "first + w + 8" in text and "ascending w" in text  # the order of the sum is written down


def test_shipped_yaml_builds_an_avg_model_config():
    import yaml

    from vit_amd.config import get_vit_config

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "exp", "finetune_avgpool.yaml")))
    assert cfg["model"]["global_pool"] == "avg" and cfg["model"]["init_from"] and cfg["model"]["task_type"] != "mim"
    assert float(cfg["model"]["drop_path_rate"]) > 0 and float(cfg["opt"]["layer_decay"]) < 1
    assert get_vit_config(copy.deepcopy(cfg)).global_pool == "avg"
    pre = yaml.safe_load(open(os.path.join(root, "configs", "exp", "mim_pretrain.yaml")))
    for k in ("image_size", "patch_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "proj_fn"):
        assert cfg["model"][k] == pre["model"][k], k  # the encoder the pre-training run hands over
