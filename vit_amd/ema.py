"""Exponential moving average of the weights, kept on the GPU (`train.ema_decay`, `train.ema_every`, `train.ema_start_step`).

The semantics are those of `torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))`: the first
update copies the parameters, every later one is `ema <- torch.lerp(ema, p, 1 - decay)`.  The state is one flat f32 buffer
shaped like the engine's flat parameter buffer (plus one per trainable parameter outside it: a trainable input preprocessor),
so an update is one launch of `vit_ema_update` over `[0, layout.n_trainable)` behind the optimizer step -- eagerly, or as the last
node of the captured step, where the weight of the replay is read from a one-float device cell -- and evaluating the average
is `vit_ema_swap`: the two buffers exchange their contents in place (the parameters are views of the flat buffer and a captured
graph holds raw addresses: data moves, addresses stay), the bf16 shadow is rewritten in the same pass.  No arithmetic runs in
PyTorch.  The averager belongs to the `Trainer`, not to the optimizer: a torch.optim optimizer is averaged just the same.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch

from . import functional as vf

__all__ = ["WeightAverager", "averaging_config", "update_due", "update_weight"]


def _int_key(config, key: str, default: int, minimum: int) -> int:
    v = config.get(key, default)
    if isinstance(v, bool) or not isinstance(v, int) or v < minimum:
        raise ValueError(f"train.{key} must be an integer >= {minimum}, got {v!r}")
    return v


def averaging_config(config) -> Optional[Dict[str, Any]]:
    """{decay, every, start_step} from the `train` section, or None without `ema_decay` (absent, null or false: no averager).
    Anything but a float strictly inside (0, 1) for the decay, an integer >= 1 / >= 0 for the other two, is a ValueError."""
    decay = config.get("ema_decay")
    if decay is None or decay is False:
        return None
    if isinstance(decay, bool) or not isinstance(decay, float) or not 0.0 < decay < 1.0:
        raise ValueError(f"train.ema_decay must be a float strictly inside (0, 1), got {decay!r}")
    return {"decay": decay, "every": _int_key(config, "ema_every", 1, 1), "start_step": _int_key(config, "ema_start_step", 0, 0)}


def update_due(step: int, every: int = 1, start_step: int = 0) -> bool:
    """Whether the average is updated after optimizer step number `step` (1-based)."""
    return step > start_step and (step - start_step) % every == 0


def update_weight(step: int, every: int, start_step: int, n_averaged: int, decay: float) -> float:
    """The lerp weight of the update after optimizer step `step`: 0 (no update), 1 (the first update: a copy) or 1 - decay,
    formed in double and rounded to f32 once where it crosses into the library, as torch rounds it."""
    if not update_due(step, every, start_step):
        return 0.0
    return 1.0 if n_averaged == 0 else 1.0 - decay


class WeightAverager:
    """The average of `model`'s trainable parameters (a MyViT) and of `extras`, trainable parameters outside its flat buffer."""

    def __init__(self, model, decay: float, every: int = 1, start_step: int = 0, extras=()):
        self.model = model
        self.decay, self.every, self.start_step = float(decay), int(every), int(start_step)
        self.extras: List[torch.nn.Parameter] = list(extras)
        self.n_averaged = 0
        self.swapped = False  # the model holds the average and `flat` the training weights (between two swap() calls)
        self.flat: Optional[torch.Tensor] = None
        self.extra_bufs: List[torch.Tensor] = []
        self.cell: Optional[torch.Tensor] = None  # [1, 4] f32, one group-table row: cell[0, 0] is a captured update's weight
        self._cell_value: Optional[float] = None  # host mirror of cell[0, 0]

    # ------------------------------------------------------------------ buffers
    def _ensure(self):
        """Zero-filled buffers like the engine's flat buffer and like every extra; one that was loaded before the model moved to
        the GPU is carried over."""
        flat = self.model.engine.flat
        if self.flat is None or self.flat.device != flat.device:
            new = torch.zeros_like(flat)
            if self.flat is not None:
                new.copy_(self.flat)
            self.flat = new
            self.cell, self._cell_value = None, None
        for i, p in enumerate(self.extras):
            cur = self.extra_bufs[i] if i < len(self.extra_bufs) else None
            if cur is None or cur.device != p.device:
                new = torch.zeros_like(p.data).contiguous().view(-1)
                if cur is not None:
                    new.copy_(cur)
                self.extra_bufs[i:i + 1] = [new]
        if self.cell is None:
            self.cell = torch.zeros(1, 4, dtype=torch.float32, device=flat.device)
            self._cell_value = 0.0

    @staticmethod
    def _storage(p) -> torch.Tensor:
        if not p.data.is_contiguous():
            raise ValueError("WeightAverager: a parameter outside the flat buffer must be contiguous")
        return p.data.view(-1)

    def _n(self) -> int:
        return self.model.engine.layout.n_trainable

    # ------------------------------------------------------------------ the schedule
    def weight_for(self, step: int) -> float:
        return update_weight(step, self.every, self.start_step, self.n_averaged, self.decay)

    def update(self, step: int) -> bool:
        """Called after optimizer step number `step` (1-based): one launch over the flat buffer, one per extra, when the
        schedule asks for an update; returns whether it did."""
        w = self.weight_for(step)
        if w == 0.0:
            return False
        if self.swapped:
            raise RuntimeError("WeightAverager.update: the model holds the averaged weights (swap() them back before training)")
        self._ensure()
        vf.ema_update(self.flat, self.model.engine.flat, w, n=self._n())
        for buf, p in zip(self.extra_bufs, self.extras):
            vf.ema_update(buf, self._storage(p), w)
        self.n_averaged += 1
        return True

    # ------------------------------------------------------------------ the captured step (vit_amd/graph.py)
    def capture_update(self):
        """Issue the update in its captured form: the weight is whatever `cell` holds when the node runs."""
        vf.ema_update(self.flat, self.model.engine.flat, weight_dev=self.cell, n=self._n())

    def set_device_weight(self, w: float) -> bool:
        """cell <- w on the current stream, ahead of a replay; a launch only when the value changed."""
        self._ensure()
        if w == self._cell_value:
            return False
        vf.ema_weight_write(self.cell, w)
        self._cell_value = w
        return True

    # ------------------------------------------------------------------ evaluation on the average
    def swap(self, engine=None):
        """Exchange the model's trainable weights with the average, in place; twice restores every bit."""
        eng = engine if engine is not None else self.model.engine
        self._ensure()
        eng._ensure_device_state()
        vf.ema_swap(eng.flat, self.flat, eng.shadow if eng.precision == "bf16" else None, n=self._n())
        eng.mark_shadow_fresh()  # the kernel rewrote flat AND shadow through raw pointers
        for buf, p in zip(self.extra_bufs, self.extras):
            vf.ema_swap(self._storage(p), buf)
        self.swapped = not self.swapped

    # ------------------------------------------------------------------ by name (HF-4.56 names, as MyViT.state_dict())
    def _extra_names(self) -> Dict[int, str]:
        return {id(p): name for name, p in self.model.named_parameters()}

    def _buffers_by_name(self) -> Dict[str, torch.Tensor]:
        """What `flat` / `extra_bufs` hold, as views by name: the trainable entries of the flat buffer and the extras."""
        self._ensure()
        lay, out = self.model.engine.layout, {}
        for name in self.model._param_names:
            if lay.entries[name][0] < lay.n_trainable:
                out[name] = lay.view(self.flat, name)
        names = self._extra_names()
        for buf, p in zip(self.extra_bufs, self.extras):
            out[names[id(p)]] = buf.view(p.shape)
        return out

    def named_states(self):
        """(averaged weights, raw training weights), each under the model's state_dict names as detached CPU clones, wherever
        the two currently are; what is not averaged (the unused pooler past n_trainable, a frozen preprocessor's buffers) is
        the model's in both."""
        held = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        other = dict(held)
        other.update({k: v.detach().cpu().clone() for k, v in self._buffers_by_name().items()})
        return (held, other) if self.swapped else (other, held)

    def averaged_state_dict(self, model=None) -> Dict[str, torch.Tensor]:
        """The averaged weights under the model's state_dict names; entries past n_trainable (the unused pooler) and whatever
        else is not averaged are the model's."""
        if model is not None and model is not self.model:
            raise ValueError("averaged_state_dict: this averager belongs to another model")
        if self.n_averaged == 0:
            raise RuntimeError("averaged_state_dict: nothing has been averaged yet")
        return self.named_states()[0]

    def train_state_dict(self) -> Dict[str, torch.Tensor]:
        """The raw training weights by name, wherever they currently are."""
        return self.named_states()[1]

    def load_averaged(self, named: Dict[str, torch.Tensor]):
        """The buffers <- the entries of `named` they average (the rest of `named` is ignored)."""
        views = self._buffers_by_name()
        missing = [k for k in views if k not in named]
        if missing:
            raise KeyError(f"WeightAverager: the averaged weights lack {missing[:3]}{'...' if len(missing) > 3 else ''}")
        with torch.no_grad():
            for k, v in views.items():
                v.copy_(named[k].reshape(v.shape))

    # ------------------------------------------------------------------ everything an update changes, for a caller that takes
    # real steps and then undoes them (Trainer._snapshot / _restore, the warm-up steps of a graph capture)
    def clone_state(self):
        return {"n_averaged": self.n_averaged, "swapped": self.swapped,
                "flat": None if self.flat is None else self.flat.clone(), "extras": [b.clone() for b in self.extra_bufs]}

    def restore_state(self, saved):
        """Buffers that existed at `clone_state()` are copied back IN PLACE (a captured graph holds their addresses); one that did
        not exist then is zeroed again, which is what a first update expects of it."""
        self.n_averaged, self.swapped = saved["n_averaged"], saved["swapped"]
        with torch.no_grad():
            olds = [saved["flat"]] + saved["extras"]
            for i, buf in enumerate(([] if self.flat is None else [self.flat]) + self.extra_bufs):
                if i < len(olds) and olds[i] is not None:
                    buf.copy_(olds[i])
                else:
                    buf.zero_()

    def state_dict(self) -> Dict[str, Any]:
        sd = {"decay": self.decay, "every": self.every, "start_step": self.start_step, "n_averaged": int(self.n_averaged)}
        if self.n_averaged > 0:
            sd["averaged"] = self.averaged_state_dict()
        return sd

    def load_state_dict(self, sd: Dict[str, Any]):
        """The counters and, when something was averaged, the averaged weights by name; decay / every / start_step stay the
        configured ones (a resumed run may change them, as it may change a learning rate)."""
        if self.swapped:
            raise RuntimeError("WeightAverager.load_state_dict: the model holds the averaged weights (swap() them back first)")
        self.n_averaged = int(sd.get("n_averaged", 0))
        if self.n_averaged > 0:
            self.load_averaged(sd["averaged"])
