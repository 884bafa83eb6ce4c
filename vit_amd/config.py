"""Config mapping of the hot path: mirrors `get_vit_config` (reference src/models/builder.py:200-258).

The reference returns a HuggingFace `ViTConfig`; the fields below are the ones the path reads, with the values the
reference hard-codes (num_channels=1, intermediate=4*hidden, erf-GELU, dropout 0.1/0.1, layer_norm_eps=1e-12,
qkv_bias=True).  Attribute names match ViTConfig so code written against the reference's config object keeps working.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

__all__ = ["ViTConfig", "get_vit_config"]


@dataclass
class ViTConfig:
    task_type: str
    image_size: int
    patch_size: int
    hidden_size: int
    num_hidden_layers: int
    num_attention_heads: int
    proj_fn: str = "SW"
    stride_ratio: float = 1
    stride_size: Optional[int] = None
    num_labels: int = 1
    num_channels: int = 1
    hidden_act: str = "gelu"
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    initializer_range: float = 0.02
    layer_norm_eps: float = 1e-12
    qkv_bias: bool = True
    pos_encoding_type: Optional[str] = None
    max_position_embeddings: int = 512
    rope_base: float = 10000.0
    # stochastic depth: layer i of L drops each of its two residual branches per sample with probability
    # linspace(0, drop_path_rate, L)[i] in training forwards (this build's key; 0 = the reference's arithmetic)
    drop_path_rate: float = 0.0
    # LayerScale: a learnable per-channel factor on each of a layer's two residual branches, initialised to this value (> 0;
    # this build's key).  None = off: the reference's model, parameter for parameter
    layer_scale_init: Optional[float] = None
    # patch dropout (timm's name and rule): a training forward keeps a random num_kept_patches of each sample's patch tokens
    # (plus CLS) and the encoder runs at that shorter sequence; evaluation sees every token (this build's key; 0 = the
    # reference's arithmetic)
    patch_drop_rate: float = 0.0
    # masked spectrum modelling (task_type 'mim', this build's key; the YAML's `mim:` section): the fraction of patch blocks a
    # forward masks, the block length in patches, the reconstruction loss ('l1' | 'mse') and MAE's per-window target
    # normalisation.  Read by a 'mim' model only.
    mim_mask_ratio: float = 0.6
    mim_span: int = 1
    mim_loss: str = "l1"
    mim_norm_target: bool = False
    # what the head reads of the final LayerNorm's output (timm's name; this build's key): 'token' = the CLS row, the
    # reference's model; 'avg' = the mean of the patch rows, CLS excluded (timm's global_pool='avg', fc_norm=False) -- how
    # SimMIM / MAE / BEiT fine-tune, since a masked objective never trains the CLS token.  No parameter is added or renamed.
    global_pool: str = "token"
    # register tokens (HF Dinov2WithRegisters' name; this build's key): R learned tokens behind CLS that take no position
    # information, that every layer attends to and every head ignores.  0 = the reference's model, parameter for parameter
    num_register_tokens: int = 0
    use_return_dict: bool = True

    def __post_init__(self):
        pool = self.global_pool
        if not isinstance(pool, str) or pool not in ("token", "avg"):
            raise ValueError(f"model.global_pool must be 'token' or 'avg' (got {pool!r})")
        if pool == "avg" and self.task_type == "mim":
            raise ValueError("model.global_pool 'avg' and model.task_type 'mim' exclude each other: a masked model decodes "
                             "every token and has no pooled head")
        rate = self.patch_drop_rate
        if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not 0.0 <= float(rate) < 1.0:
            raise ValueError(f"patch_drop_rate must lie in [0, 1) (got {rate!r})")
        reg = self.num_register_tokens
        if isinstance(reg, bool) or not isinstance(reg, int) or reg < 0:
            raise ValueError(f"model.num_register_tokens must be an integer >= 0 (got {reg!r})")
        if reg > 0 and float(rate) > 0.0:
            raise ValueError(f"model.num_register_tokens ({reg}) together with model.patch_drop_rate ({rate}) is not built yet: "
                             f"the gather forms of the embedding kernels take no register rows")
        if self.task_type == "mim":
            ratio, span = self.mim_mask_ratio, self.mim_span
            if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 < float(ratio) < 1.0:
                raise ValueError(f"mim.mask_ratio must lie in (0, 1) (got {ratio!r})")
            if isinstance(span, bool) or not isinstance(span, int) or span < 1:
                raise ValueError(f"mim.span must be an integer >= 1 (got {span!r})")
            if self.mim_loss not in ("l1", "mse"):
                raise ValueError(f"mim.loss must be 'l1' or 'mse' (got {self.mim_loss!r})")
            if not isinstance(self.mim_norm_target, bool):
                raise ValueError(f"mim.norm_target must be true or false (got {self.mim_norm_target!r})")
            if float(rate) > 0.0:
                raise ValueError(f"model.patch_drop_rate ({rate}) and model.task_type 'mim' exclude each other: both draw their "
                                 f"patch selection from the same site, and a masked model runs at every token")

    @property
    def intermediate_size(self) -> int:  # builder.py:243
        return 4 * self.hidden_size

    @property
    def stride(self) -> int:  # embedding.py:25-26
        s = self.stride_size
        return int(s) if s and s > 0 else int(self.stride_ratio * self.patch_size)

    @property
    def num_patches(self) -> int:
        L, P, S = self.image_size, self.patch_size, self.stride
        if self.proj_fn == "SW":  # tokenization.py:40
            return math.ceil((L - P) / S) + 1
        if self.proj_fn in ("C1D", "CNN"):  # tokenization.py:65
            return (L - P) // S + 1
        raise ValueError(f"Unsupported proj_fn '{self.proj_fn}'")  # embedding.py:44

    @property
    def seq_len(self) -> int:
        """T = 1 + R + N: CLS, the register tokens, the patches."""
        return self.num_patches + 1 + self.num_register_tokens

    @property
    def num_kept_patches(self) -> int:
        """K of patch dropout: max(1, int(N * (1 - patch_drop_rate))) in Python doubles, as timm's PatchDropout computes it."""
        return kept_patches(self.num_patches, self.patch_drop_rate)

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads


def kept_patches(num_patches: int, rate: float) -> int:
    """How many of `num_patches` patch tokens a training forward keeps at patch_drop_rate `rate` (ValueError outside [0, 1))."""
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"patch_drop_rate must lie in [0, 1) (got {rate})")
    return max(1, int(num_patches * (1.0 - rate)))


def mim_blocks(num_patches: int, span: int, mask_ratio: float):
    """(Nb, Kb) of masked spectrum modelling: the patches fall into Nb = ceil(N / span) blocks of `span` consecutive patches (the
    last one may be short), of which Kb = max(1, int(Nb * (1 - mask_ratio))) stay visible -- kept_patches' expression."""
    nb = -(-int(num_patches) // int(span))
    return nb, max(1, int(nb * (1.0 - float(mask_ratio))))


def _targets_in(param) -> int:
    """How many regression targets `data.param` names: a comma-separated string or a list; anything else (None, '', []) = 1."""
    if isinstance(param, str):
        names = [tok for tok in (piece.strip() for piece in param.split(",")) if tok]
        return len(names) or 1
    if isinstance(param, (list, tuple)):
        return len(param) or 1
    return 1


def get_vit_config(config) -> ViTConfig:
    """The model config from the YAML dict (reference: src/models/builder.py:200-258, pinned on it by
    tests/golden/config.json).  Regression: `num_labels` ALWAYS follows `data.param` -- a conflicting `model.num_labels` is
    overridden with a warning -- and is written back into config['model']; classification takes `model.num_labels`."""
    import warnings

    model = config["model"]
    task = str(model.get("task_type") or model.get("task") or "cls").lower()
    if task in ("reg", "regression"):
        num_labels = _targets_in((config.get("data") or {}).get("param"))
        stated = model.get("num_labels")
        if stated is not None and int(stated) != num_labels:
            warnings.warn(f"model.num_labels={stated} disagrees with data.param, which names {num_labels} target(s); "
                          f"using {num_labels}", stacklevel=2)
        model["num_labels"] = num_labels
    else:
        num_labels = int(model.get("num_labels", 1) or 1)
    optional = {k: model[k] for k in ("stride_ratio", "stride_size", "pos_encoding_type", "max_position_embeddings", "rope_base",
                                      "drop_path_rate", "layer_scale_init", "patch_drop_rate", "global_pool", "num_register_tokens")
                if k in model}
    if task == "mim":
        # the `mim:` section: {mask_ratio, span, loss, norm_target}; anything else in it is a spelling mistake
        section = dict(config.get("mim") or {})
        unknown = sorted(set(section) - {"mask_ratio", "span", "loss", "norm_target"})
        if unknown:
            raise ValueError(f"mim: unknown key(s) {unknown}; the section takes mask_ratio, span, loss, norm_target")
        if "loss" in section:
            section["loss"] = str(section["loss"]).lower()
        optional.update({"mim_" + k: v for k, v in section.items()})
        if (config.get("augment") or {}).get("mixup_alpha") or (config.get("augment") or {}).get("cutmix_alpha"):
            raise ValueError("augment (Mixup / CutMix) and model.task_type 'mim' exclude each other: a masked model has no "
                             "labels to mix, and its target is the signal it was given")
        model["task_type"] = task
    return ViTConfig(
        task_type=model["task_type"], image_size=model["image_size"], patch_size=model["patch_size"],
        hidden_size=model["hidden_size"], num_hidden_layers=model["num_hidden_layers"],
        num_attention_heads=model["num_attention_heads"], proj_fn=model["proj_fn"], num_labels=num_labels, **optional)
