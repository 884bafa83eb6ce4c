"""Mixup / CutMix of a training batch (`augment:` in the config; include/vit_amd_mix.h, vit_amd/csrc/mix.hip).

timm's `Mixup` restated for 1-D spectra.  The partner of sample b in a batch of B is B - 1 - b; Mixup is a convex combination of
the two spectra, CutMix replaces a contiguous wavelength span [lo, hi) by the partner's.  Regression labels mix linearly, class
labels become soft targets over the (optionally label-smoothed) one-hot rows.  What is mixed is DRAWN ON THE HOST, per training
call, as a plan of rows (w, u, lo, hi, wy, uy) -- one for the batch (`mode: batch`) or one per sample (`mode: elem`):

  1. with probability `prob` the row mixes, otherwise it is the identity (1, 0, 0, 0, 1, 0);
  2. if both alphas are > 0, CutMix is chosen with probability `switch_prob` (one alpha > 0: that branch);
  3. lam ~ Beta(a, a) with that branch's alpha;
  4. Mixup:  w = wy = f32(lam), u = uy = f32(1 - lam) (subtracted in double), lo = hi = 0;
  5. CutMix: cut = int(L * (1 - lam)), c = integers(0, L), lo = clip(c - cut // 2, 0, L), hi = clip(c + cut // 2, 0, L),
     w = 1, u = 0, wy = f32(1 - (hi - lo) / L), uy = f32((hi - lo) / L)   (timm's correct_lam).

The randomness is counter-based: call n of a mixer draws from numpy.random.default_rng([seed, rank, n]), so the mixer's only
state is n and a resumed run continues the sequence exactly without a saved generator.  The plan reaches the device in kernel
arguments (vit_mix_plan_write) and two launches apply it on the current stream: vit_mix_signal and vit_mix_targets.  Evaluation
never mixes.  timm's `pair` mode, `cutmix_minmax` and mixing across ranks are not included.
"""
from __future__ import annotations

import math
import os
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

__all__ = ["Mixup", "IDENTITY_ROW", "augment_config", "mixup_from_config"]

Row = Tuple[float, float, int, int, float, float]  # (w, u, lo, hi, wy, uy); the floats are exact f32 values
IDENTITY_ROW: Row = (1.0, 0.0, 0, 0, 1.0, 0.0)
MODES = ("batch", "elem")
SOFT_LOSSES = ("ce", "bce")
_DEFAULTS = {"mixup_alpha": 0.0, "cutmix_alpha": 0.0, "prob": 1.0, "switch_prob": 0.5, "mode": "batch", "label_smoothing": 0.0,
             "soft_loss": None, "seed": 0}


def _f32(v: float) -> float:
    return float(np.float32(v))


class Mixup:
    def __init__(self, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0, switch_prob: float = 0.5,
                 mode: str = "batch", label_smoothing: float = 0.0, num_classes: Optional[int] = None, seed: int = 0,
                 rank: int = 0):
        """`num_classes` None: regression labels (mixed linearly); else int64 class labels -> soft targets [B, num_classes]."""
        for name, a in (("mixup_alpha", mixup_alpha), ("cutmix_alpha", cutmix_alpha)):
            if isinstance(a, bool) or not isinstance(a, (int, float)) or not math.isfinite(a) or a < 0:
                raise ValueError(f"augment.{name} must be a finite number >= 0, got {a!r}")
        for name, v in (("prob", prob), ("switch_prob", switch_prob)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:
                raise ValueError(f"augment.{name} must lie in [0, 1], got {v!r}")
        if mode not in MODES:
            raise ValueError(f"augment.mode must be one of {MODES} (timm's 'pair' is not included), got {mode!r}")
        s = label_smoothing
        if isinstance(s, bool) or not isinstance(s, (int, float)) or not 0.0 <= s < 1.0:
            raise ValueError(f"augment.label_smoothing must lie in [0, 1), got {s!r}")
        if s and num_classes is None:
            raise ValueError("augment.label_smoothing needs class labels (model.task_type: cls)")
        if num_classes is not None and (isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 1):
            raise ValueError(f"num_classes must be a positive integer or None, got {num_classes!r}")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.mode = float(prob), float(switch_prob), mode
        self.label_smoothing, self.num_classes = float(s), num_classes
        self.seed, self.rank = int(seed), int(rank)
        self.n = 0  # training calls drawn so far: the whole state
        self.last_rows: Optional[List[Row]] = None  # the plan of the last apply()
        self._plans: Dict[Any, Any] = {}  # device -> (plan buffer, its row capacity, the identity plan)

    # ------------------------------------------------------------------ host side: the draw
    def _draw_row(self, rng, L: int) -> Row:
        if not rng.random() < self.prob:
            return IDENTITY_ROW
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cutmix = bool(rng.random() < self.switch_prob)
        elif self.mixup_alpha > 0 or self.cutmix_alpha > 0:
            cutmix = self.cutmix_alpha > 0
        else:
            return IDENTITY_ROW
        a = self.cutmix_alpha if cutmix else self.mixup_alpha
        lam = float(rng.beta(a, a))
        if not cutmix:
            return (_f32(lam), _f32(1.0 - lam), 0, 0, _f32(lam), _f32(1.0 - lam))
        cut = int(L * (1.0 - lam))
        c = int(rng.integers(0, L))
        lo, hi = min(max(c - cut // 2, 0), L), min(max(c + cut // 2, 0), L)
        share = (hi - lo) / L
        return (1.0, 0.0, lo, hi, _f32(1.0 - share), _f32(share))

    def draw(self, B: int, L: int) -> List[Row]:
        """The plan of the next training call on a batch [B, L]: one row (`batch`) or B rows (`elem`).  Host only."""
        if B < 1 or L < 1:
            raise ValueError(f"Mixup.draw: B = {B}, L = {L} must be positive")
        rng = np.random.default_rng([self.seed, self.rank, self.n])
        self.n += 1
        return [self._draw_row(rng, L) for _ in range(B if self.mode == "elem" else 1)]

    def on_off(self) -> Tuple[float, float]:
        """The two values of a smoothed one-hot row, formed in double (rounded once where they cross the C ABI)."""
        if self.num_classes is None:
            return 1.0, 0.0
        off = self.label_smoothing / self.num_classes
        return 1.0 - self.label_smoothing + off, off

    def state_dict(self) -> Dict[str, int]:
        return {"n": int(self.n)}

    def load_state_dict(self, state) -> None:
        self.n = int(state["n"])

    # ------------------------------------------------------------------ device side
    def _plan(self, device, n_rows: int):
        import torch

        from . import functional as vf

        slot = self._plans.get(device)
        if slot is None or slot[1] < n_rows:
            ident = slot[2] if slot is not None else None
            if ident is None:
                ident = torch.zeros(vf.MIX_ROW_BYTES, dtype=torch.uint8, device=device)
                vf.mix_plan_write(ident, [IDENTITY_ROW])
            slot = (torch.zeros(n_rows * vf.MIX_ROW_BYTES, dtype=torch.uint8, device=device), n_rows, ident)
            self._plans[device] = slot
        return slot

    def _labels(self, labels):
        import torch

        if self.num_classes is None:
            return labels.to(torch.float32).contiguous()
        if labels.dtype != torch.int64 or labels.dim() != 1:
            raise ValueError(f"Mixup: class labels must be int64 [B], got {labels.dtype} {tuple(labels.shape)}")
        return labels.contiguous()

    def apply(self, flux, labels, out_x=None, out_y=None):
        """Draw the next plan and mix (flux [B, L] f32, labels) by it on the current stream -> (x, y).  `flux` and `labels`
        are only read (a loader may hand out views of its dataset) unless `out_x is flux`, the in-place form -- for a tensor
        the caller owns, such as the one vit_add_noise returned.  Without `out_x` / `out_y` the results are fresh tensors."""
        import torch

        from . import functional as vf

        if flux.dim() != 2:
            raise ValueError(f"Mixup.apply: flux must be [B, L], got {tuple(flux.shape)}")
        x = flux if flux.dtype == torch.float32 and flux.is_contiguous() else flux.to(torch.float32).contiguous()
        if x.data_ptr() % 16:  # a view into a dataset whose rows are not 16-byte multiples: the kernels want an aligned base
            x = x.clone()
        if out_x is flux and x is not flux:
            raise ValueError("Mixup.apply: the in-place form needs a contiguous, 16-byte-aligned f32 flux")
        B, L = x.shape
        rows = self.draw(B, L)
        plan, _, _ = self._plan(x.device, len(rows))
        vf.mix_plan_write(plan, rows)
        self.last_rows = rows
        out = vf.mix_signal(x, plan, len(rows), out=out_x)
        on, off = self.on_off()
        y = vf.mix_targets(self._labels(labels), plan, len(rows), self.num_classes, on, off, out=out_y)
        return out, y

    def targets_like(self, labels):
        """The targets an identity plan gives `labels` (their shape and dtype as apply() returns them; with label smoothing:
        the smoothed one-hot rows).  Consumes no draw."""
        from . import functional as vf

        on, off = self.on_off()
        _, _, ident = self._plan(labels.device, 1)
        return vf.mix_targets(self._labels(labels), ident, 1, self.num_classes, on, off)


def augment_config(config) -> Optional[Dict[str, Any]]:
    """The validated `augment` block of a run's config, or None when it is absent or switches nothing on (no mixing, no label
    smoothing).  Raises ValueError for a block the run cannot honour -- also one that switches nothing on."""
    block = config.get("augment") if hasattr(config, "get") else None
    if block is None:
        return None
    if not hasattr(block, "items"):
        raise ValueError(f"augment must be a mapping, got {block!r}")
    unknown = sorted(set(block) - set(_DEFAULTS))
    if unknown:
        raise ValueError(f"augment: unknown key(s) {unknown}; known: {sorted(_DEFAULTS)}")
    a = dict(_DEFAULTS)
    a.update({k: v for k, v in block.items() if v is not None})
    model = config.get("model") or {}
    task = str(model.get("task_type") or model.get("task") or "cls").lower()
    cls = task in ("classification", "cls", "class")
    if a["soft_loss"] is not None and a["soft_loss"] not in SOFT_LOSSES:
        raise ValueError(f"augment.soft_loss must be one of {SOFT_LOSSES}, got {a['soft_loss']!r}")
    if not cls and a["soft_loss"] is not None:
        raise ValueError("augment.soft_loss needs class labels (model.task_type: cls); a regression run mixes its labels linearly")
    if not cls and a["label_smoothing"]:
        raise ValueError("augment.label_smoothing needs class labels (model.task_type: cls)")
    if isinstance(a["seed"], bool) or not isinstance(a["seed"], int) or a["seed"] < 0:
        raise ValueError(f"augment.seed must be an integer >= 0, got {a['seed']!r}")
    num_classes = int(model.get("num_labels", 1) or 1) if cls else None
    # the constructor checks the numbers; a block that passes and switches nothing on builds nothing
    Mixup(a["mixup_alpha"], a["cutmix_alpha"], a["prob"], a["switch_prob"], a["mode"], a["label_smoothing"], num_classes, a["seed"])
    if not (a["mixup_alpha"] or a["cutmix_alpha"] or a["label_smoothing"]):
        return None
    a["num_classes"] = num_classes
    a["soft_loss"] = (a["soft_loss"] or "ce") if cls else None
    return a


def mixup_from_config(config, num_classes: Optional[int] = None, rank: Optional[int] = None) -> Optional[Mixup]:
    """The run's mixer, or None (the default: no object is built and no launch is made).  `num_classes`: the model's own count
    for a classification run (it overrides model.num_labels of the config)."""
    a = augment_config(config)
    if a is None:
        return None
    if a["num_classes"] is not None and num_classes is not None:
        a["num_classes"] = int(num_classes)
    rank = int(os.environ.get("RANK", "0")) if rank is None else int(rank)
    m = Mixup(a["mixup_alpha"], a["cutmix_alpha"], a["prob"], a["switch_prob"], a["mode"], a["label_smoothing"], a["num_classes"],
              a["seed"], rank)
    m.soft_loss = a["soft_loss"]
    return m
