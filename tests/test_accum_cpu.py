"""Host side of gradient accumulation (`train.accumulate_grad_batches`, vit_handle_set_option "grad_accumulate"): what can be
checked without a GPU.  The kernels, the autograd node and the trainer's steps are tests/test_accum_gpu.py's."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config(**train):
    cfg = {
        "model": dict(name="vit", task_type="reg", image_size=512, patch_size=32, hidden_size=32, num_hidden_layers=1,
                      num_attention_heads=2, stride_size=32, proj_fn="SW"),
        "train": dict(batch_size=4, ep=2, precision="32"),
        "loss": {"name": "mae"}, "opt": {"type": "AdamW", "lr": 1e-3, "lr_sch": "onecycle"},
        "data": {"param": "log_g", "num_samples": 40}, "noise": {"noise_level": 0},
    }
    cfg["train"].update(train)
    return cfg


@pytest.mark.parametrize("bad", [0, -1, 2.5, 4.0, "4", None, True, [4]])
def test_accumulate_grad_batches_must_be_a_positive_integer(bad):
    from vit_amd.trainer import Trainer

    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        Trainer(config(accumulate_grad_batches=bad)["train"], device=torch.device("cpu"), verbose=False)


def test_accumulate_grad_batches_default_and_values():
    from vit_amd.trainer import Trainer

    assert Trainer(config()["train"], device=torch.device("cpu"), verbose=False).accumulate_grad_batches == 1
    for k in (1, 2, 7):
        t = Trainer(config(accumulate_grad_batches=k)["train"], device=torch.device("cpu"), verbose=False)
        assert t.accumulate_grad_batches == k and t._micro == 0


@pytest.mark.parametrize("num_samples,batch_size,K,steps", [(40, 4, None, 10), (40, 4, 1, 10), (40, 4, 4, 3), (41, 4, 4, 3),
                                                            (48, 4, 4, 3), (49, 4, 4, 4), (40, 16, 2, 2), (3, 4, 8, 1)])
def test_one_cycle_counts_optimizer_steps(num_samples, batch_size, K, steps):
    """steps_per_epoch = ceil(ceil(num_samples / batch_size) / K): the scheduler steps once per optimizer step, and a short
    trailing group still steps.  K = 1 and the key absent: the batches of an epoch, as before."""
    from vit_amd.module import ViTLModule

    cfg = config(batch_size=batch_size, **({} if K is None else {"accumulate_grad_batches": K}))
    cfg["data"]["num_samples"] = num_samples
    conf = ViTLModule(config=cfg).configure_optimizers()
    assert conf["lr_scheduler"]["interval"] == "step"
    assert conf["lr_scheduler"]["scheduler"].total_steps == steps * cfg["train"]["ep"]


def test_last_batch_is_flagged_with_one_batch_of_look_ahead():
    from vit_amd.trainer import _flag_last

    assert list(_flag_last([])) == []
    assert list(_flag_last(["a"])) == [("a", True)]
    assert list(_flag_last(iter("abc"))) == [("a", False), ("b", False), ("c", True)]
    pulled = []

    def source():
        for i in range(3):
            pulled.append(i)
            yield i

    it = _flag_last(source())
    assert next(it) == (0, False) and pulled == [0, 1]  # exactly one item ahead


def test_header_lists_grad_accumulate_among_the_handle_options():
    text = open(os.path.join(ROOT, "include", "vit_amd.h")).read()
    decl = text.index("int vit_handle_set_option(")
    comment = text[text.rindex("/*", 0, decl):decl]
    assert '"reserve_cus"' in comment and '"grad_accumulate"' in comment
    # the comment of vit_layernorm_bwd speaks of the option, not of a parameter the function does not have
    ln = text[text.rindex("/*", 0, text.index("int vit_layernorm_bwd(")):text.index("int vit_layernorm_bwd(")]
    assert "grad_accumulate" in ln and not re.search(r"accumulate\s*!=\s*0", ln)
    # and the library's option table knows the name
    api = open(os.path.join(ROOT, "vit_amd", "csrc", "api.hip")).read()
    body = api[api.index("int vit_handle_set_option("):]
    assert 'strcmp(name, "grad_accumulate")' in body[:body.index("\nint ", 10)]


def test_disarmed_reducer_ignores_bucket_callbacks():
    """Lightning's no_sync on the micro-batches that are not followed by an optimizer step: bucket_ready returns before it
    touches the gradient buffer or the process group."""
    from vit_amd.ddp import GradAllReducer

    def never():
        raise AssertionError("a disarmed reducer read the gradient buffer")

    red = GradAllReducer(never, [(0, 8), (8, 24)])
    red.active = True  # as under a process group
    red.armed = False
    red.bucket_ready(0, 8)
    assert red.collectives == 0 and red._pending == []
    red.finish()
