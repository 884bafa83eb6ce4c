"""A model and its engine refer to each other, so a dropped model is freed by Python's cycle collector, not by its last
reference going away.  Its activation arena, gradients and workspaces must not wait for whenever that collector next runs
(in the middle of another model's step, say): the engine runs it before it allocates a new arena (ViTEngine._ensure_arena)."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_a_dropped_models_memory_is_released_before_the_next_arena_is_allocated(dev):
    from test_cls_tail_gpu import build, case

    rc, sd, flux, labels, _, _ = case("l1")
    x, y = flux.to(dev), labels.to(dev)

    def one_step():
        model = build(rc, sd, dev, "bf16-mixed").train()
        model(x, labels=y).loss.backward()
        torch.cuda.synchronize()
        return model

    gc.collect()
    before = torch.cuda.memory_allocated()
    gc.disable()  # from here on only an explicit collection frees a cycle: what the engine does is what is measured
    try:
        first = one_step()
        one = torch.cuda.memory_allocated() - before  # what one live model holds: parameters, arena, gradients, workspaces
        assert one > 0
        del first
        second = one_step()  # its first forward allocates an arena: the dropped model goes first
        two = torch.cuda.memory_allocated() - before
        assert two <= 1.1 * one, (one, two)
        del second
    finally:
        gc.enable()
        gc.collect()
