"""`MyViT`: drop-in for the reference's model class (src/models/specvit.py:16-115) on MI355X.

Same constructor arguments, `forward(pixel_values, labels=None, output_attentions=None, output_hidden_states=None,
return_dict=None)` returning an object with `.loss / .logits / .hidden_states / .attentions`, same `.name`,
`.loss_name`, `compute_loss`, `log_outputs`, `set_preprocessor_trainable`, the same ValueError for a bad task_type, and
a `state_dict()` whose keys are those of the reference's checkpoints (transformers 4.56 module names), so checkpoints
move in both directions.  All arithmetic runs in libvit_amd.so; parameters are views of one flat fp32 buffer.
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Any, Optional, Tuple

import torch
import torch.nn as nn

from ._cabi import VitError
from .config import ViTConfig
from .engine import ViTEngine

__all__ = ["MyViT", "SequenceClassifierOutput", "build_model_name"]


@dataclass
class SequenceClassifierOutput:
    """Field-compatible with transformers.modeling_outputs.SequenceClassifierOutput (attribute, key and index access)."""

    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    attentions: Optional[Tuple[torch.Tensor, ...]] = None

    def to_tuple(self):
        return tuple(getattr(self, f.name) for f in fields(self) if getattr(self, f.name) is not None)

    def __getitem__(self, k):
        return getattr(self, k) if isinstance(k, str) else self.to_tuple()[k]

    def get(self, k, default=None):
        v = getattr(self, k, None)
        return default if v is None else v

    def keys(self):
        return [f.name for f in fields(self) if getattr(self, f.name) is not None]


@dataclass
class MaskedModelingOutput(SequenceClassifierOutput):
    """What a 'mim' model returns: HF MaskedImageModelingOutput's `loss` / `reconstruction` [B, N, P] / `hidden_states` /
    `attentions`, plus the `mask` [B, N] (int32, non-zero = masked) the forward used.  `logits` is the reconstruction too, so
    code written against the other tasks' output keeps reading a prediction.  `reconstruction` and `mask` are views of the
    engine's activation arena: the next forward of the same mode overwrites them (clone what has to outlive it)."""

    reconstruction: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None


def build_model_name(config, model_prefix: str = "ViT", full_config: dict = None) -> str:
    """Run name `{prefix}_p{patch}_h{hidden}_l{layers}_a{heads}_s{stride}_p{proj_fn}[_nz{noise digits}][_mim][_gap][_reg{R}]` -- the rule of
    src/models/model_utils.py:9-45 (pinned by tests/golden/names.json).  The stride tag is the explicit `stride_size` when
    one is set (truthy), else the `stride_ratio`; a positive noise level is appended with its decimal point removed; a masked
    spectrum model (task_type 'mim', this build's) appends `_mim`, a model whose head reads the mean of the patch tokens
    (global_pool 'avg', this build's) `_gap` -- two runs that differ in pooling alone do not share a checkpoint directory."""
    explicit = getattr(config, "stride_size", None)
    fields = [
        ("p", config.patch_size), ("h", config.hidden_size), ("l", config.num_hidden_layers),
        ("a", config.num_attention_heads), ("s", int(explicit) if explicit else config.stride_ratio), ("p", config.proj_fn),
    ]
    name = "_".join([model_prefix] + [f"{tag}{value}" for tag, value in fields])
    level = ((full_config or {}).get("noise") or {}).get("noise_level", 0)
    if level and level > 0:
        name += "_nz" + str(level).replace(".", "")
    if getattr(config, "task_type", None) == "mim":
        name += "_mim"
    if getattr(config, "global_pool", "token") == "avg":
        name += "_gap"
    if int(getattr(config, "num_register_tokens", 0) or 0) > 0:  # register tokens (this build's): `_reg{R}`
        name += f"_reg{int(config.num_register_tokens)}"
    return name


class _Node(nn.Module):
    """Structural container: only exists so parameters get the reference's dotted names."""


def _trunc_normal_(t: torch.Tensor, std: float):
    nn.init.trunc_normal_(t, mean=0.0, std=std, a=-2.0, b=2.0)


class _ViTFunction(torch.autograd.Function):
    """Whole-model autograd node: forward/backward are the engine's kernel sequences; parameter gradients come back as
    views of the engine's flat gradient buffer (no copies when .grad is None, i.e. zero_grad(set_to_none=True)).

    A second backward without zero_grad in between (gradient accumulation: Lightning's accumulate_grad_batches, the plain
    `loss.backward()` idiom) finds those views as the parameters' `.grad`.  Returning them again would make autograd run
    `p.grad += <the same memory>` after the kernels overwrote it -- twice the last micro-batch's gradient.  So when every
    trainable parameter still holds its view, the kernels ADD into the buffer (ViTEngine.backward(accumulate=True)) and
    autograd gets None for them.

    With a `SharpnessAware` attached (MyViT.set_sam, vit_amd/sam.py) the backward is the whole two-pass step: the first
    eng.backward (silent towards the gradient exchange), ascend, a second forward on the node's own input with the first one's
    random draws, the second eng.backward with the same dloss (this one is exchanged), descend -- the last in a `finally`, so no
    exception leaves perturbed weights behind.  The flat gradient buffer then holds the gradient at the perturbed weights."""

    @staticmethod
    def forward(ctx, model, x, labels, training, keep_hidden, *params):
        eng = model.engine
        if model._sam is not None:
            if x.requires_grad:
                raise ValueError("sharpness-aware minimisation (set_sam / train.sam_rho) does not cover an input that requires "
                                 "grad (a trainable input preprocessor)")
            # what the second pass needs to be the same function at other weights: the input, and the caller's selections
            ctx.sam_args = (x, labels, training, keep_hidden, eng.mim_mask, eng.patch_keep)
        # keep_hidden: the caller reads eng.act["x"] afterwards, so the engine has to know BEFORE it runs that the last
        # layer's token rows are wanted (otherwise it computes that layer's CLS rows only: ViTEngine.cls_tail)
        loss, logits, model._kept_hidden, _ = eng.forward(x, labels, training=training, need_grad=True,
                                                          output_hidden_states=keep_hidden)
        ctx.model = model
        ctx.gen = eng._gen
        ctx.need_dx = bool(x.requires_grad)  # a trainable input preprocessor in front of the ViT
        if model._sam is not None and eng.mim:
            logits = logits.clone()  # a view of the arena's mim_pred: the second pass overwrites it
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        model = ctx.model
        eng = model.engine
        # frozen parameters and the pooler (its output is never used, specvit.py:78: no gradient, as in the reference) get None
        live = [p.requires_grad and not name.startswith("vit.pooler.") for name, p in zip(model._param_names, model._param_list)]
        held = [ok and eng.grads is not None and p.grad is not None and p.grad.data_ptr() == eng.g(name).data_ptr()
                for ok, name, p in zip(live, model._param_names, model._param_list)]
        accumulate = any(held)
        if accumulate and held != live:
            # the fused kernels write q / k / v and the LayerNorm / bias groups together: one mode for the whole buffer
            bad = next(n for n, ok, h in zip(model._param_names, live, held) if ok and not h)
            raise VitError(f"backward: {bad}.grad is not the flat gradient buffer's view while other parameters still hold "
                           f"theirs from an earlier backward; gradients accumulate in place for all trainable parameters or "
                           f"for none -- call zero_grad() on the whole model (set_to_none=True or False), not on single parameters")
        sam = model._sam
        if sam is not None and hasattr(ctx, "sam_args"):
            if accumulate:
                raise VitError("backward: gradients would accumulate into an earlier backward's (no zero_grad in between) while "
                               "sharpness-aware minimisation is attached; the two-pass step does not cover accumulation")
            _ViTFunction._sam_backward(ctx, model, sam, dloss)
            dx = None
        else:
            dx = eng.backward(dloss, need_dx=ctx.need_dx, gen=ctx.gen, accumulate=accumulate)
        grads = [eng.g(name) if ok and not accumulate else None for ok, name in zip(live, model._param_names)]
        return (None, dx, None, None, None, *grads)

    @staticmethod
    def _sam_backward(ctx, model, sam, dloss):
        eng = model.engine
        x, labels, training, keep_hidden, mim_mask, patch_keep = ctx.sam_args
        cb, eng.grad_ready_cb = eng.grad_ready_cb, None  # the first gradient stays local: only the second one is exchanged
        try:
            eng.backward(dloss, gen=ctx.gen)
        finally:
            eng.grad_ready_cb = cb
        held = (eng.mim_mask, eng.patch_keep)
        try:
            sam.ascend()
            eng.mim_mask, eng.patch_keep = mim_mask, patch_keep
            with torch.no_grad():
                eng.forward(x, labels, training=training, need_grad=True, output_hidden_states=keep_hidden, reuse_step=True)
            eng.backward(dloss)
        finally:
            eng.mim_mask, eng.patch_keep = held
            sam.descend()


class MyViT(nn.Module):
    """Vision Transformer over 1-D spectra (reference: `MyViT(ViTPreTrainedModel, BaseModel)`)."""

    config_class = ViTConfig

    def __init__(self, config: ViTConfig, loss_name: str = "", model_name: str = "ViT",
                 preprocessor: Optional[nn.Module] = None, full_config: dict = None) -> None:
        super().__init__()
        self.config = config
        self.task_type = config.task_type
        if self.task_type not in ("cls", "reg", "mim"):
            raise ValueError(f"Unsupported task_type '{self.task_type}'")  # specvit.py:55
        self.preprocessor = preprocessor  # specvit.py:43, 72-73: applied to pixel_values before the ViT
        self.engine = ViTEngine(config, loss_name=loss_name)
        self._kept_hidden = None
        self._sam = None  # a SharpnessAware (set_sam): the autograd node's backward then runs the two-pass step
        self._loss_name = self.engine.loss_name
        self._name_args = (model_name, full_config)
        self._model_name = build_model_name(config, model_name, full_config=full_config)
        self._build_tree()
        self.init_weights()

    # ------------------------------------------------------------------ structure
    def _build_tree(self):
        lay = self.engine.layout
        self._param_names = list(lay.state_order)
        plist = []
        for name in self._param_names:
            parts = name.split(".")
            node = self
            for part in parts[:-1]:
                if part not in node._modules:
                    node.add_module(part, _Node())
                node = node._modules[part]
            prm = nn.Parameter(lay.view(self.engine.flat, name), requires_grad=True)
            node.register_parameter(parts[-1], prm)
            plist.append(prm)
        self._param_list = plist
        self.engine.version_fn = self._version_signature

    def _version_signature(self) -> int:
        # in-place updates by torch optimizers / load_state_dict / p.copy_() bump the parameter's version counter
        return sum(p._version for p in self._param_list) + self.engine.flat._version

    def _rebind_views(self):
        lay = self.engine.layout
        for name, prm in zip(self._param_names, self._param_list):
            prm.data = lay.view(self.engine.flat, name)
            prm.grad = None

    def _apply(self, fn, recurse=True):
        """.to()/.cuda()/.cpu(): move the ONE flat buffer and re-point every parameter at its slice."""
        new_flat = fn(self.engine.flat)
        self.engine.rebind(new_flat)
        self._rebind_views()
        if self.preprocessor is not None:
            self.preprocessor._apply(fn)
        return self

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=False)
        self.engine._shadow_version = -1
        return out

    @torch.no_grad()
    def init_weights(self):
        """HF `_init_weights` as the reference triggers it (specvit.py:57): Linear / Conv weights ~ trunc_normal(0,
        initializer_range), biases 0, LayerNorm 1/0.  cls_token and learned position_embeddings belong to
        SpectraEmbeddings (not an HF ViTEmbeddings), so they keep their torch.randn values (embedding.py:47,62-64).
        `register_tokens` (model.num_register_tokens > 0) ~ N(0, initializer_range^2), drawn AFTER every other tensor: a model
        with registers starts from the values the same config and seed give every other tensor without them.  timm starts its
        registers at std 1e-6; initializer_range is this project's choice (HF Dinov2WithRegisters starts them at zero, where
        identical registers receive identical gradients and stay identical for ever)."""
        std = self.config.initializer_range
        registers = None
        for name, p in zip(self._param_names, self._param_list):
            if name.endswith("register_tokens"):
                registers = p
            elif name.endswith("cls_token") or name.endswith("position_embeddings"):
                p.copy_(torch.randn(p.shape))
            elif name.endswith("mask_token"):  # task_type 'mim': HF ViTEmbeddings starts it at zero
                p.zero_()
            elif name.endswith(".lambda1"):  # LayerScale (config.layer_scale_init): present only when the feature is on
                p.fill_(float(self.config.layer_scale_init))
            elif "layernorm" in name:
                p.fill_(1.0 if name.endswith("weight") else 0.0)
            elif name.endswith("bias"):
                p.zero_()
            else:
                _trunc_normal_(p, std)
        if registers is not None:
            registers.copy_(torch.randn(registers.shape) * std)

    # ------------------------------------------------------------------ reference surface
    @property
    def name(self):
        return self._model_name

    @property
    def loss_name(self):
        return self._loss_name

    def set_global_pool(self, mode: str):
        """Switch what the head reads, 'token' (the CLS row) or 'avg' (the mean of the patch rows): no tensor changes its name
        or shape, so this is all it takes to evaluate a checkpoint under the pooling it was trained with.  The run name follows."""
        self.engine.set_global_pool(mode)
        self._model_name = build_model_name(self.config, self._name_args[0], full_config=self._name_args[1])

    def set_sam(self, rho, adaptive: bool = False):
        """Attach sharpness-aware minimisation (vit_amd/sam.py): from now on every `loss.backward()` through this model leaves
        the gradient at the perturbed weights w + e(w) in the flat gradient buffer and the weights restored.  `rho=None` detaches.
        Returns the SharpnessAware (or None)."""
        from .sam import SharpnessAware

        if self._sam is not None and self._sam.perturbed:
            raise RuntimeError("set_sam: the model holds perturbed weights")
        self._sam = None if rho is None else SharpnessAware(self, rho, adaptive)
        return self._sam

    @property
    def sam(self):
        return self._sam

    def train(self, mode: bool = True):
        """eval() (= train(False)) also restarts a 'mim' model's evaluation-mask counter (see forward)."""
        if not mode:
            self.engine.reset_mim_eval()
        return super().train(mode)

    def forward(self, pixel_values, labels=None, output_attentions=None, output_hidden_states=None, return_dict=None,
                bool_masked_pos=None):
        """A 'mim' model (masked spectrum modelling) ignores `labels` and returns a MaskedModelingOutput: `.loss`, the
        reconstruction loss over the masked windows; `.reconstruction` [B, N, P]; `.mask` [B, N]; `.hidden_states`;
        `.attentions`.  `bool_masked_pos` (HF's name): a bool / integer [B, N] device tensor, non-zero = masked, used as given.
        None draws the mask on the device: in training mode from the step's seed (a fresh mask per step); in eval mode from
            seed_k = ((base_seed ^ 0x6D696D5F6576616C) + 0x9E3779B97F4A7C15 * (k + 1)) mod 2^64,
        k = the number of mask-drawing eval forwards since the last eval() / train(False) call -- a function of the engine's
        base_seed and that counter alone, never of the batch contents, so every validation epoch that starts with eval() sees
        the same masks in the same order.  The other tasks take no `bool_masked_pos`."""
        eng = self.engine
        training = self.training
        if self.preprocessor is not None:
            pixel_values = self.preprocessor(pixel_values)
        mim = self.task_type == "mim"
        if bool_masked_pos is not None and not mim:
            raise ValueError("bool_masked_pos belongs to masked spectrum modelling (model.task_type 'mim')")
        if mim:
            labels = None
            held, eng.mim_mask = eng.mim_mask, bool_masked_pos if bool_masked_pos is not None else eng.mim_mask
            try:
                return self._forward(pixel_values, labels, training, output_attentions, output_hidden_states, return_dict)
            finally:
                eng.mim_mask = held
        return self._forward(pixel_values, labels, training, output_attentions, output_hidden_states, return_dict)

    def _forward(self, pixel_values, labels, training, output_attentions, output_hidden_states, return_dict):
        eng = self.engine
        mim = self.task_type == "mim"
        # forward hooks on `vit.encoder.layer.N.attention.attention` (what the reference's viz callback registers to read
        # attention maps, src/viz/viz_callback.py:183-214, 231-235): the kernels have no per-layer Python forward to hook,
        # so when such hooks exist the maps are produced anyway and the hooks are called with HF's (context, probs) output
        hooked = self._hooked_attention_layers()
        if hooked:
            output_attentions_user, output_attentions = output_attentions, True
        want_grad = torch.is_grad_enabled() and (labels is not None or mim) and any(p.requires_grad for p in self._param_list)
        ctxs = [] if hooked else None
        if want_grad:
            # the loss stays differentiable whatever else is asked for (as in the reference); hidden states / attention maps
            # are read back from the activations that forward kept (maps: the probabilities before dropout)
            loss, logits = _ViTFunction.apply(self, pixel_values, labels, training, bool(output_hidden_states),
                                              *self._param_list)
            hs, self._kept_hidden = self._kept_hidden, None  # copies of eng.act["x"], or None when not asked for
            atts = eng.saved_attentions() if output_attentions else None
            if hooked:
                # the forward's own sequence length: 1 + K tokens under patch dropout
                B, T, D = pixel_values.shape[0], eng._last["T"], self.config.hidden_size
                ctxs = [c.view(B, T, D) for c in eng.act["ctx"]]
        else:
            with torch.no_grad():
                loss, logits, hs, atts = eng.forward(pixel_values, labels, training=training, need_grad=False,
                                                     output_hidden_states=bool(output_hidden_states),
                                                     output_attentions=bool(output_attentions), capture_ctx=ctxs)
        if hooked:
            for i in hooked:
                node = self._attention_node(i)
                for hook in list(node._forward_hooks.values()):
                    hook(node, (), (ctxs[i].detach(), atts[i]))
            if not output_attentions_user:
                atts = None
        hs, atts = tuple(hs) if hs is not None else None, tuple(atts) if atts is not None else None
        if mim:
            mask = eng._last["mask"]
            if want_grad and self._sam is not None:
                mask = mask.clone()  # the arena's: the second pass of a sharpness-aware backward writes it again
            out = MaskedModelingOutput(loss=loss, logits=logits, hidden_states=hs, attentions=atts, reconstruction=logits,
                                       mask=mask)
        else:
            out = SequenceClassifierOutput(loss=loss, logits=logits, hidden_states=hs, attentions=atts)
        if return_dict is False:
            return out.to_tuple()
        return out

    def _attention_node(self, i: int):
        return self._modules["vit"]._modules["encoder"]._modules["layer"]._modules[str(i)]._modules["attention"]._modules["attention"]

    def _hooked_attention_layers(self):
        return [i for i in range(self.config.num_hidden_layers) if self._attention_node(i)._forward_hooks]

    def compute_loss(self, *args, **kwargs):
        return self.forward(*args, **kwargs).loss

    def log_outputs(self, outputs, log_fn=print, stage: str = ""):
        loss = outputs.get("loss") if isinstance(outputs, dict) else getattr(outputs, "loss", None)
        if loss is not None:
            log_fn({f"{self.loss_name}_loss": loss})

    def set_preprocessor_trainable(self, trainable: bool) -> None:
        """specvit.py:118-130: freeze / unfreeze the input preprocessor."""
        if self.preprocessor is None:
            return
        if hasattr(self.preprocessor, "set_qk_trainable"):
            self.preprocessor.set_qk_trainable(trainable)
        elif hasattr(self.preprocessor, "freeze"):
            self.preprocessor.freeze(not trainable)
        else:
            for param in self.preprocessor.parameters():
                param.requires_grad = trainable

    def set_precision(self, precision) -> str:
        """'32' (reference default; fp32-class kernels) or 'bf16-mixed' (bf16 MFMA operands): see ViTEngine."""
        if self.preprocessor is not None and hasattr(self.preprocessor, "set_precision"):
            self.preprocessor.set_precision(precision)
        return self.engine.set_precision(precision)

    # ------------------------------------------------------------------ extras used by the build's own trainer
    def flat_parameters(self) -> torch.Tensor:
        return self.engine.flat

    def flat_gradients(self) -> torch.Tensor:
        return self.engine.grads
