"""Sharpness-aware minimisation on the GPU (`train.sam_rho`, `train.sam_adaptive`): the two-pass step of Foret et al. 2021 (SAM) and,
with `sam_adaptive`, of Kwon et al. 2021 (ASAM), in the elementwise form of the widely used davda54/sam.

One optimisation step on a batch with weights w:
  1. g = grad L(w): forward + backward as ever;
  2. ascend: w' = w + rho * c * g / (||a * g|| + 1e-12), c = w^2 and a = |w| in the adaptive form, 1 otherwise; the norm runs over
     every perturbed element;
  3. g_sam = grad L(w') on the same batch with the same random draws (dropout masks, drop-path gates, patch-dropout selection,
     `mim` mask): the second forward reads the first one's step seed;
  4. descend: w is restored bit for bit; clip and optimizer step with g_sam.
Steps 2 and 4 are streaming launches over the flat buffers (include/vit_amd_sam.h): the norm by the deterministic two-stage
reduction of the clip norm, the ascent (which keeps w in one flat f32 backup buffer and rewrites the bf16 shadow in the same pass)
and the descent.  The norm never visits the host.  The model's autograd node runs steps 2-4 behind its first backward
(vit_amd/specvit.py), so a plain `loss.backward()` leaves g_sam in the flat gradient buffer whoever calls it; the captured step
states the same sequence explicitly (vit_amd/graph.py).  Under data parallelism every rank perturbs by its local gradient
(m-sharpness) and only the second backward is exchanged.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import functional as vf

__all__ = ["SharpnessAware", "sam_config"]


def sam_config(config) -> Optional[Dict[str, Any]]:
    """{rho, adaptive} from the `train` section, or None without `sam_rho` (absent or null: nothing is attached).  A rho that is
    not a finite number > 0, a non-bool `sam_adaptive`, or `sam_adaptive` without `sam_rho` is a ValueError."""
    rho, adaptive = config.get("sam_rho"), config.get("sam_adaptive")
    if adaptive is not None and not isinstance(adaptive, bool):
        raise ValueError(f"train.sam_adaptive must be a bool, got {adaptive!r}")
    if rho is None:
        if adaptive:
            raise ValueError("train.sam_adaptive needs train.sam_rho")
        return None
    if isinstance(rho, bool) or not isinstance(rho, (int, float)) or not math.isfinite(rho) or not rho > 0:
        raise ValueError(f"train.sam_rho must be a finite number > 0, got {rho!r}")
    return {"rho": float(rho), "adaptive": bool(adaptive)}


class SharpnessAware:
    """The perturbation of `model`'s (a MyViT) live parameters: `ascend()` after the first backward, `descend()` after the second."""

    def __init__(self, model, rho: float, adaptive: bool = False):
        if isinstance(rho, bool) or not isinstance(rho, (int, float)) or not math.isfinite(rho) or not rho > 0:
            raise ValueError(f"SharpnessAware: rho must be a finite number > 0, got {rho!r}")
        self.model = model
        self.rho, self.adaptive = float(rho), bool(adaptive)
        self.perturbed = False  # between ascend() and descend(): the model holds w', `backup` holds w
        self.backup: Optional[torch.Tensor] = None
        self.last_grad_norm: Optional[torch.Tensor] = None  # device scalar: the SQUARED norm of step 2, as the optimizer's clip keeps it
        self._sq: Optional[torch.Tensor] = None
        self._runs: List[Tuple[int, int]] = []  # what the last ascend() perturbed: descend() restores exactly that

    def _ensure(self):
        """The backup, one flat f32 buffer like the engine's, and the norm's cell, on the engine's device."""
        flat = self.model.engine.flat
        if self.backup is None or self.backup.device != flat.device:
            if self.perturbed:
                raise RuntimeError("SharpnessAware: the model moved while it held perturbed weights")
            self.backup = torch.zeros_like(flat)
            self._sq = torch.zeros(1, dtype=torch.float32, device=flat.device)

    def runs(self) -> List[Tuple[int, int]]:
        """Contiguous [lo, hi) runs of the flat buffer whose parameters are live in this backward -- requires_grad, not the
        pooler, below layout.n_trainable (the rule of _ViTFunction.backward / FusedOptimizer._active_ranges) -- ascending; the
        alignment pad behind an entry belongs to it."""
        model, lay = self.model, self.model.engine.layout
        spans = []
        for name, p in zip(model._param_names, model._param_list):
            off, _ = lay.entries[name]
            if off >= lay.n_trainable or not p.requires_grad or name.startswith("vit.pooler."):
                continue
            spans.append((off, off + (lay.numel(name) + 7) // 8 * 8))
        spans.sort()
        runs: List[List[int]] = []
        for a, b in spans:
            if runs and runs[-1][1] == a:
                runs[-1][1] = b
            else:
                runs.append([a, b])
        return [(a, b) for a, b in runs]

    def _shadow(self, eng):
        return eng.shadow if eng.precision == "bf16" else None

    def ascend(self, runs: Optional[List[Tuple[int, int]]] = None):
        """w -> w' from the gradient in the engine's flat gradient buffer: the norm over `runs` (default: the live runs) in
        ascending order, then one ascent launch per run.  Nothing is read back."""
        if self.perturbed:
            raise RuntimeError("SharpnessAware.ascend: the weights are already perturbed (descend() first)")
        eng = self.model.engine
        eng._ensure_device_state()
        self._ensure()
        runs = self.runs() if runs is None else list(runs)
        sq, shadow = self._sq, self._shadow(eng)
        with vf.use_handle(eng.handle()):
            first = True
            for a, b in runs:
                vf.sam_sqnorm(eng.grads[a:b], eng.flat[a:b], adaptive=self.adaptive, accumulate=not first, out=sq)
                first = False
            if first:
                sq.zero_()
            self.last_grad_norm = sq
            self._runs = runs
            self.perturbed = True  # from the first launch on: a failure in between still restores
            for a, b in runs:
                vf.sam_ascend(eng.flat[a:b], eng.grads[a:b], self.backup[a:b], None if shadow is None else shadow[a:b], self.rho,
                              sq, adaptive=self.adaptive)
        eng.mark_shadow_fresh()  # the kernel rewrote flat AND shadow through raw pointers; LayerScale refolds from w'

    def descend(self):
        """w' -> w, bit for bit, over the runs the last ascend() perturbed.  Nothing happens when nothing is perturbed."""
        if not self.perturbed:
            return
        eng = self.model.engine
        shadow = self._shadow(eng)
        with vf.use_handle(eng.handle()):
            for a, b in self._runs:
                vf.sam_descend(eng.flat[a:b], self.backup[a:b], None if shadow is None else shadow[a:b])
        self.perturbed = False
        eng.mark_shadow_fresh()  # LayerScale refolds from the restored w
