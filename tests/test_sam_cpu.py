"""Sharpness-aware minimisation without a GPU: `sam_config` and the Trainer's refusals, the three exports (header, ctypes
prototypes, the built library), the host restatement (tests/_sam_ref.py) against a direct torch statement of davda54/sam's first
step, the oracle's two passes, and the shipped YAML."""
import math
import os

import numpy as np
import pytest
import torch

import _sam_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"vit_sam_sqnorm": 8, "vit_sam_ascend": 10, "vit_sam_descend": 6}  # name -> arguments, the handle included


def test_sam_config_cases():
    from vit_amd.sam import sam_config

    assert sam_config({}) is None
    assert sam_config({"sam_rho": None}) is None
    assert sam_config({"sam_rho": None, "sam_adaptive": False}) is None
    assert sam_config({"sam_rho": 0.05}) == {"rho": 0.05, "adaptive": False}
    assert sam_config({"sam_rho": 2, "sam_adaptive": True}) == {"rho": 2.0, "adaptive": True}
    assert isinstance(sam_config({"sam_rho": 2})["rho"], float)
    for bad in (0, 0.0, -0.1, float("nan"), float("inf"), -float("inf"), True, False, "0.05", [0.05]):
        with pytest.raises(ValueError, match="sam_rho"):
            sam_config({"sam_rho": bad})
    with pytest.raises(ValueError, match="sam_adaptive needs"):
        sam_config({"sam_adaptive": True})
    for bad in (1, "yes", 0.5):
        with pytest.raises(ValueError, match="sam_adaptive must be a bool"):
            sam_config({"sam_rho": 0.05, "sam_adaptive": bad})


def test_trainer_refuses_accumulation_and_bad_values():
    from vit_amd.trainer import Trainer

    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        Trainer({"sam_rho": 0.05, "accumulate_grad_batches": 2}, device=dev, verbose=False)
    with pytest.raises(ValueError, match="sam_rho"):
        Trainer({"sam_rho": -1.0}, device=dev, verbose=False)
    with pytest.raises(ValueError, match="sam_adaptive"):
        Trainer({"sam_adaptive": True}, device=dev, verbose=False)
    assert Trainer({"sam_rho": 0.05}, device=dev, verbose=False).sam_cfg == {"rho": 0.05, "adaptive": False}
    assert Trainer({"accumulate_grad_batches": 2}, device=dev, verbose=False).sam_cfg is None


def test_sharpness_aware_constructor_and_live_runs():
    from oracle import refvit
    from vit_amd.config import ViTConfig
    from vit_amd.sam import SharpnessAware
    from vit_amd.specvit import MyViT

    rc = refvit.named_config("C1")
    model = MyViT(ViTConfig(task_type=rc.task_type, image_size=rc.image_size, patch_size=rc.patch_size, hidden_size=rc.hidden_size,
                            num_hidden_layers=rc.num_hidden_layers, num_attention_heads=rc.num_attention_heads,
                            stride_size=rc.stride_size))
    for bad in (0, -1.0, float("nan"), True, None, "1"):
        with pytest.raises(ValueError, match="rho"):
            SharpnessAware(model, bad)
    assert model.sam is None
    sam = model.set_sam(0.05, adaptive=True)
    assert model.sam is sam and sam.rho == 0.05 and sam.adaptive is True and sam.perturbed is False and sam.backup is None
    lay = model.engine.layout
    assert sam.runs() == [(0, lay.n_trainable)]  # everything but the pooler, one run
    # frozen tensors leave the runs: the query and key weights of layer 1
    frozen = ["vit.encoder.layer.1.attention.attention.query.weight", "vit.encoder.layer.1.attention.attention.key.weight"]
    for name, p in zip(model._param_names, model._param_list):
        if name in frozen:
            p.requires_grad_(False)
    lo = lay.entries[frozen[0]][0]
    hi = lay.entries[frozen[1]][0] + lay.numel(frozen[1])
    assert sam.runs() == [(0, lo), (hi, lay.n_trainable)]
    assert model.set_sam(None) is None and model.sam is None


def test_header_declares_the_three_exports_and_the_binding_knows_them():
    from vit_amd import _cabi
    from vit_amd.build import HEADERS, SOURCES

    names = _cabi.declared_symbols()
    lib = _cabi.load()
    for n, argc in EXPORTS.items():
        assert n in names and len(_cabi._PROTOS[n]) == argc and hasattr(lib, n), n
    assert "sam.hip" in SOURCES and any(h.endswith("vit_amd_sam.h") for h in HEADERS)
    text = open(os.path.join(ROOT, "include", "vit_amd_sam.h")).read()
    assert '#include "vit_amd_sam.h"' in open(os.path.join(ROOT, "include", "vit_amd.h")).read()
    for said in ("16 (+2) B per parameter", "8 (+2) B per parameter", "1e-12", "Non-finite norm"):
        assert said in text, said


@pytest.mark.parametrize("adaptive", [False, True])
def test_restatement_is_davda_sams_first_step(adaptive):
    gen = torch.Generator().manual_seed(5)
    shapes = [(7, 5), (13,), (3, 4, 2), (1,)]
    params = [torch.randn(s, generator=gen) * 0.3 for s in shapes]
    grads = [torch.randn(s, generator=gen) * 2.0 for s in shapes]
    rho = 0.5 if adaptive else 0.05
    want = sr.davda_first_step([p.double() for p in params], [g.double() for g in grads], rho, adaptive)
    sd = {f"p{i}": p for i, p in enumerate(params)}
    eps = sr.named_epsilon(sd, {f"p{i}": g for i, g in enumerate(grads)}, rho, adaptive)
    sq = sum(sr.sqnorm(p.numpy(), g.numpy(), adaptive) for p, g in zip(params, grads))
    for i, (p, g, w) in enumerate(zip(params, grads, want)):
        e = eps[f"p{i}"].double()
        assert float((p.double() + e - w).norm() / w.norm()) < 1e-6
        assert float((e - (w - p.double())).norm() / (w - p.double()).norm()) < 1e-6  # the step itself, not only p + step
        assert np.array_equal(sr.ascend(p.numpy(), g.numpy(), rho, adaptive, sq), (p + eps[f"p{i}"]).numpy())
    flat_e = torch.cat([e.flatten() for e in eps.values()]).double()
    if not adaptive:  # the plain step has length rho
        assert abs(float(flat_e.norm()) - rho) < 1e-6 * rho
    # a zero gradient is a zero step
    assert not sr.epsilon(params[0].numpy(), np.zeros(shapes[0], np.float32), rho, adaptive, sq=1.0).any()


def test_oracle_sam_runs_the_second_pass_at_the_perturbed_weights():
    from oracle import dropmask as dm
    from oracle import refvit

    rc = refvit.RefConfig(image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, stride_size=32,
                          loss_name="mae")
    sd = refvit.make_state_dict(rc, 3)
    flux, _, labels = refvit.make_inputs(rc, 3, 4)
    masks = dm.engine_masks(rc.hidden_dropout_prob, rc.attention_probs_dropout_prob, dm.step_seed(17, 2), None)
    o = sr.oracle_sam(rc, sd, flux, labels, masks, 0.05, False)
    assert set(o["g"]) == set(o["g_sam"]) == set(o["eps"]) and "vit.pooler.dense.weight" not in o["g"]
    e = torch.cat([v.flatten() for v in o["eps"].values()]).double()
    assert abs(float(e.norm()) - 0.05) < 1e-6
    cat = lambda d: torch.cat([d[k].flatten() for k in sorted(d)]).double()  # noqa: E731
    apart = float((cat(o["g_sam"]) - cat(o["g"])).norm() / cat(o["g_sam"]).norm())
    assert apart > 1e-3 and math.isfinite(o["loss_sam"]) and o["loss_sam"] != o["loss"]
    # with eps given: the same second pass, no first one
    again = sr.oracle_sam(rc, sd, flux, labels, masks, 0.05, False, eps=o["eps"])
    assert again["g"] is None and again["loss"] is None and again["loss_sam"] == o["loss_sam"]
    assert all(torch.equal(again["g_sam"][k], o["g_sam"][k]) for k in o["g_sam"])
    # SAM ascends: to first order L(w + e) - L(w) = rho * ||g|| > 0
    assert o["loss_sam"] > o["loss"]


def test_the_yaml_loads():
    import copy

    import yaml

    from vit_amd.config import get_vit_config
    from vit_amd.sam import sam_config

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "exp", "sam_scratch.yaml")))
    assert sam_config(cfg["train"]) == {"rho": 0.05, "adaptive": False}
    assert cfg["train"]["hip_graph"] is True and cfg["opt"]["type"] == "AdamW" and cfg["model"]["task_type"] == "cls"
    assert "init_from" not in cfg["model"]  # from scratch
    assert get_vit_config(copy.deepcopy(cfg)).num_labels == 10
