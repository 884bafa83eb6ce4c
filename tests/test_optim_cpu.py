"""CPU suite of the fused SGD / Adam-L2 steps: the new C entry points refuse bad arguments with a status and a message (no
GPU touched), and the optimizer factory resolves the reference's three documented `opt.type`s (src/opt/optimizer.py:14-26,108;
configs/config.yaml) to the fused classes for a MyViT while everything else resolves as before."""
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from vit_amd import _cabi
    from vit_amd import build as vb

    vb.build(force=False, verbose=False)
    return _cabi.load()


P = 0x1000  # a non-null "device pointer": every call below must fail its argument check before it could be used


def _err(lib, rc, *needles):
    assert rc == -1, rc
    msg = lib.vit_last_error().decode()
    for n in needles:
        assert n in msg, msg


def test_sgd_step_argument_errors(lib):
    #                   h     p  g  buf   pb    n  lr   mom  wd  nest sq   max  stream
    _err(lib, lib.vit_sgd_step(None, None, P, None, None, 8, 0.1, 0.0, 0.0, 0, None, 0.0, None), "vit_sgd_step", "null")
    _err(lib, lib.vit_sgd_step(None, P, None, None, None, 8, 0.1, 0.0, 0.0, 0, None, 0.0, None), "vit_sgd_step", "null")
    _err(lib, lib.vit_sgd_step(None, P, P, None, None, 0, 0.1, 0.0, 0.0, 0, None, 0.0, None), "n = 0")
    _err(lib, lib.vit_sgd_step(None, P, P, None, None, -4, 0.1, 0.0, 0.0, 0, None, 0.0, None), "n = -4")
    _err(lib, lib.vit_sgd_step(None, P, P, None, None, 8, 0.1, 0.9, 0.0, 0, None, 0.0, None), "momentum buffer")
    _err(lib, lib.vit_sgd_step(None, P, P, P, None, 8, 0.1, -0.5, 0.0, 0, None, 0.0, None), "negative")
    _err(lib, lib.vit_sgd_step(None, P, P, None, None, 8, 0.1, 0.0, 0.0, 1, None, 0.0, None), "nesterov")


def test_adam_l2_step_argument_errors(lib):
    args = (8, 1e-3, 0.9, 0.999, 1e-8, 0.01)
    _err(lib, lib.vit_adam_l2_step(None, None, P, P, P, None, *args, 1, None, 0.0, None), "vit_adam_l2_step")
    _err(lib, lib.vit_adam_l2_step(None, P, None, P, P, None, *args, 1, None, 0.0, None), "vit_adam_l2_step")
    _err(lib, lib.vit_adam_l2_step(None, P, P, P, P, None, 0, *args[1:], 1, None, 0.0, None), "vit_adam_l2_step")
    _err(lib, lib.vit_adam_l2_step(None, P, P, P, P, None, *args, 0, None, 0.0, None), "vit_adam_l2_step")  # step < 1


def test_dyn_forms_need_a_bound_record(lib):
    """The by-value entry points have no `_dyn` form: a captured step goes through the `_groups_dyn` forms, whose refusal without
    a bound record is asserted in tests/test_optim_groups_cpu.py."""
    from vit_amd import _cabi

    for name in ("vit_sgd_step", "vit_adam_l2_step"):
        assert name in _cabi._PROTOS and name in _cabi.declared_symbols()
    assert len(_cabi._PROTOS["vit_adam_l2_step"]) == len(_cabi._PROTOS["vit_adamw_step"])
    for name in ("vit_adamw_step_dyn", "vit_adam_l2_step_dyn", "vit_sgd_step_dyn"):
        assert name not in _cabi._PROTOS and name not in _cabi.declared_symbols()


@pytest.fixture(scope="module")
def vit():
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    cfg = ViTConfig(task_type="reg", image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=1, num_attention_heads=2,
                    stride_size=32, num_labels=1)
    return MyViT(cfg, loss_name="mae")


def _opt(conf):
    return conf["optimizer"] if isinstance(conf, dict) else conf


def test_factory_resolves_sgd_and_adam_with_decay_to_the_fused_classes(vit):
    from vit_amd.optimizer import FusedAdamW, FusedOptimizer, FusedSGD, OptModule

    sgd = _opt(OptModule.from_config({"type": "SGD", "lr": 1e-2, "weight_decay": 0.01})(vit))
    assert type(sgd) is FusedSGD and isinstance(sgd, FusedOptimizer)
    g = sgd.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"]) == (1e-2, 0, 0, 0.01, False)
    ref = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    assert set(g) == set(ref.param_groups[0])  # schedulers and torch.optim.SGD.load_state_dict find every key
    assert not hasattr(sgd, "_m") and not hasattr(sgd, "_v") and sgd._buf is None
    assert sgd.state_dict()["state"] == {}

    l2 = _opt(OptModule.from_config({"type": "Adam", "weight_decay": 0.01})(vit))
    assert type(l2) is FusedAdamW and l2.adam_l2 is True and l2.param_groups[0]["weight_decay"] == 0.01


def test_one_cycle_gives_fused_sgd_a_momentum(vit):
    from vit_amd.optimizer import FusedSGD, OptModule

    conf = OptModule.from_config({"type": "SGD", "lr": 1e-2, "lr_sch": "onecycle", "steps_per_epoch": 4, "epochs": 2})(vit)
    assert type(conf["optimizer"]) is FusedSGD
    assert conf["optimizer"].param_groups[0]["momentum"] == pytest.approx(0.95)


def test_factory_resolves_everything_else_as_before(vit):
    from vit_amd.optimizer import FusedAdamW, OptModule

    adam = _opt(OptModule.from_config({"type": "Adam"})(vit))
    assert type(adam) is FusedAdamW and adam.adam_l2 is False and adam.param_groups[0]["weight_decay"] == 0
    adamw = _opt(OptModule.from_config({"type": "AdamW", "weight_decay": 0.01})(vit))
    assert type(adamw) is FusedAdamW and adamw.adam_l2 is False and adamw.param_groups[0]["weight_decay"] == 0.01
    assert set(adamw.param_groups[0]) == {"params", "lr", "betas", "eps", "weight_decay"}
    assert type(_opt(OptModule.from_config({"type": "RMSprop"})(vit))) is torch.optim.RMSprop
    lin = torch.nn.Linear(4, 2)  # not a MyViT: torch's own classes, whatever the type
    assert type(_opt(OptModule.from_config({"type": "SGD"})(lin))) is torch.optim.SGD
    assert type(_opt(OptModule.from_config({"type": "Adam", "weight_decay": 0.01})(lin))) is torch.optim.Adam


def test_fused_sgd_refuses_what_it_does_not_implement(vit):
    from vit_amd.optimizer import FusedSGD

    with pytest.raises(ValueError, match="dampening"):
        FusedSGD(vit, lr=1e-2, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError, match="[Nn]esterov"):
        FusedSGD(vit, lr=1e-2, nesterov=True)  # torch.optim.SGD refuses it too
    with pytest.raises(ValueError):
        FusedSGD(vit, lr=1e-2, momentum=-0.1)
