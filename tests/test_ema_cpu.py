"""Host side of the weights' exponential moving average (`train.ema_decay`, include/vit_amd_ema.h, vit_amd/ema.py): what can be
checked without a GPU.  The kernels, the averager and the trainer's use of it are tests/test_ema_gpu.py's."""
import ctypes

import pytest
import torch


def config(**train):
    cfg = {
        "model": dict(name="vit", task_type="reg", image_size=512, patch_size=32, hidden_size=32, num_hidden_layers=1,
                      num_attention_heads=2, stride_size=32, proj_fn="SW"),
        "train": dict(batch_size=4, ep=2, precision="32"),
        "loss": {"name": "mae"}, "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"}, "noise": {"noise_level": 0},
    }
    cfg["train"].update(train)
    return cfg


def test_ema_symbols_are_exported_and_prototyped():
    from vit_amd import _cabi
    from vit_amd import build as vb

    vb.build(force=False, verbose=False)
    lib = _cabi.load()
    declared = _cabi.declared_symbols()
    for sym in ("vit_ema_update", "vit_ema_swap"):
        assert sym in declared, f"{sym} is not declared by a header vit_amd.h includes"
        assert hasattr(lib, sym), f"{sym} declared but not exported"
        assert sym in _cabi._PROTOS, f"{sym} has no ctypes prototype"
    assert set(_cabi._PROTOS) == set(declared)
    assert lib.vit_version() == 100


def test_ema_argument_errors_launch_nothing():
    """Every refusal comes back as VIT_ERR_ARG (-1) with a message, from the checks in front of the launch: the pointers below
    are not device memory (there is no GPU), so a call that got as far as a launch would not return -1."""
    from vit_amd import _cabi

    lib = _cabi.load()
    a, b = 0x10000, 0x20000  # 16-byte aligned, never dereferenced

    def refused(rc, *words):
        assert rc == -1
        msg = lib.vit_last_error().decode()
        assert all(w in msg for w in words), msg

    refused(lib.vit_ema_update(None, None, b, 8, 0.1, None, None), "vit_ema_update", "null")
    refused(lib.vit_ema_update(None, a, None, 8, 0.1, None, None), "vit_ema_update", "null")
    refused(lib.vit_ema_update(None, a, b, 0, 0.1, None, None), "vit_ema_update", "n = 0")
    refused(lib.vit_ema_update(None, a, b, -4, 0.1, None, None), "vit_ema_update", "n = -4")
    refused(lib.vit_ema_update(None, a + 4, b, 8, 0.1, None, None), "vit_ema_update", "16-byte")
    refused(lib.vit_ema_update(None, a, b + 8, 8, 0.1, None, None), "vit_ema_update", "16-byte")
    refused(lib.vit_ema_update(None, a, b, 8, 1.5, None, None), "vit_ema_update", "weight = 1.5")
    refused(lib.vit_ema_update(None, a, b, 8, -0.25, None, None), "vit_ema_update", "weight = -0.25")
    refused(lib.vit_ema_update(None, a, b, 8, float("nan"), None, None), "vit_ema_update", "weight")
    refused(lib.vit_ema_update(None, a, b, 8, float("inf"), None, None), "vit_ema_update", "weight")
    refused(lib.vit_ema_update(None, a, b, 8, 0.1, a + 4, None), "vit_ema_update", "weight_dev")
    refused(lib.vit_ema_swap(None, None, b, None, 8, None), "vit_ema_swap", "null")
    refused(lib.vit_ema_swap(None, a, None, None, 8, None), "vit_ema_swap", "null")
    refused(lib.vit_ema_swap(None, a, b, None, 0, None), "vit_ema_swap", "n = 0")
    refused(lib.vit_ema_swap(None, a + 4, b, None, 8, None), "vit_ema_swap", "16-byte")
    refused(lib.vit_ema_swap(None, a, b + 12, None, 8, None), "vit_ema_swap", "16-byte")
    refused(lib.vit_ema_swap(None, a, b, 0x30002, 8, None), "vit_ema_swap", "p_bf16")


def test_weight_crosses_the_abi_already_subtracted():
    """1 - decay is formed in double and rounded once where ctypes hands it to the library: float(1 - 0.999) is 0.001f, which
    1.f - 0.999f is not (the `one_minus` note of include/vit_amd_optim.h)."""
    from vit_amd.ema import update_weight

    w = update_weight(1, 1, 0, 5, 0.999)
    once = ctypes.c_float(w).value
    assert once == ctypes.c_float(0.001).value
    assert once != ctypes.c_float(ctypes.c_float(1.0).value - ctypes.c_float(0.999).value).value
    assert once == float(torch.tensor(1 - 0.999, dtype=torch.float32))


def test_trainer_builds_no_averager_without_the_key():
    from vit_amd.trainer import Trainer

    for train in ({}, {"ema_decay": None}, {"ema_decay": False}, {"ema_every": 3, "ema_start_step": 7}):
        t = Trainer(config(**train)["train"], device=torch.device("cpu"), verbose=False)
        assert t.ema_cfg is None and t.averager is None
    t = Trainer(config(ema_decay=0.99)["train"], device=torch.device("cpu"), verbose=False)
    assert t.ema_cfg == {"decay": 0.99, "every": 1, "start_step": 0} and t.averager is None  # built with the optimizer, in _setup
    t = Trainer(config(ema_decay=0.5, ema_every=4, ema_start_step=0)["train"], device=torch.device("cpu"), verbose=False)
    assert t.ema_cfg == {"decay": 0.5, "every": 4, "start_step": 0}


@pytest.mark.parametrize("bad", [0.0, 1.0, 1.5, -0.1, 1, 0, True, "0.99", [0.9], float("nan"), float("inf")])
def test_ema_decay_must_be_a_float_inside_the_unit_interval(bad):
    from vit_amd.trainer import Trainer

    with pytest.raises(ValueError, match="ema_decay"):
        Trainer(config(ema_decay=bad)["train"], device=torch.device("cpu"), verbose=False)


@pytest.mark.parametrize("key,bad", [("ema_every", 0), ("ema_every", -2), ("ema_every", 2.0), ("ema_every", "2"), ("ema_every", True),
                                     ("ema_every", None), ("ema_start_step", -1), ("ema_start_step", 1.5),
                                     ("ema_start_step", "0"), ("ema_start_step", False), ("ema_start_step", None)])
def test_ema_every_and_start_step_must_be_integers_in_range(key, bad):
    from vit_amd.trainer import Trainer

    with pytest.raises(ValueError, match=key):
        Trainer(config(ema_decay=0.9, **{key: bad})["train"], device=torch.device("cpu"), verbose=False)


# (every, start_step) -> the optimizer steps (1-based) among 1..12 after which the average is updated, written out by hand:
# s > start_step and (s - start_step) % every == 0
SCHEDULE = {
    (1, 0): [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12],
    (2, 0): [2, 4, 6, 8, 10, 12],
    (3, 0): [3, 6, 9, 12],
    (1, 3): [4, 5, 6, 7, 8, 9, 10, 11, 12],
    (2, 3): [5, 7, 9, 11],
    (3, 4): [7, 10],
    (5, 7): [12],
    (1, 12): [],
    (13, 0): [],
}


@pytest.mark.parametrize("every,start_step", sorted(SCHEDULE))
def test_update_schedule_against_a_hand_written_table(every, start_step):
    from vit_amd.ema import update_due, update_weight

    decay = 0.9
    assert [s for s in range(1, 13) if update_due(s, every, start_step)] == SCHEDULE[(every, start_step)]
    # the weights of a run: 0 on a skipped step, 1 for the first update (a copy), 1 - decay from then on
    n_averaged, weights = 0, []
    for s in range(1, 13):
        w = update_weight(s, every, start_step, n_averaged, decay)
        weights.append(w)
        n_averaged += w != 0.0
    due = SCHEDULE[(every, start_step)]
    want = [0.0 if s not in due else 1.0 if s == due[0] else 1.0 - decay for s in range(1, 13)]
    assert weights == want and n_averaged == len(due)
    assert update_due(0, every, start_step) is False  # nothing before the first optimizer step


def test_averager_follows_the_schedule_without_touching_a_buffer_on_skipped_steps():
    """On a step the schedule skips, update() returns before it asks for device memory (the model here sits on the CPU)."""
    from vit_amd.ema import WeightAverager
    from vit_amd.module import ViTLModule

    model = ViTLModule(config=config()).model
    avg = WeightAverager(model, 0.9, every=2, start_step=3)
    for s in (1, 2, 3, 4, 6):
        assert avg.update(s) is False
    assert avg.n_averaged == 0 and avg.flat is None and avg.weight_for(5) == 1.0
    with pytest.raises(RuntimeError, match="nothing has been averaged"):
        avg.averaged_state_dict(model)
