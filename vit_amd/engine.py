"""Host-side engine of the ViT step: owns the flat parameter / gradient buffers and the activation arena in HBM and
sequences the HIP kernels of libvit_amd.so (through vit_amd.functional -> ctypes -> C ABI) for forward and backward.

Data layout in HBM (one MI355X, 288 GB: nothing is recomputed or re-materialised to save memory)
  params   f32 [n_total]   flat; every tensor of the reference's state_dict (transformers-4.56 names) is a view.
                           query/key/value weights (and biases) of a layer are adjacent, so the fused QKV projection
                           reads them as one [3D, D] matrix.  Pooler last (never receives a gradient: specvit.py:78).
  shadow   bf16 [n_total]  same offsets; what the MFMA GEMMs read.  Refreshed by the fused AdamW kernel, or by one cast
                           pass whenever the f32 buffer was modified behind our back (load_state_dict, a torch optimizer).
  grads    f32 [n_total]   same offsets; every kernel that produces a parameter gradient writes its slice exactly once --
                           or, in a backward with accumulate=True, adds to it exactly once (gradient accumulation over
                           micro-batches: the kernels' final stores read the old value).
  arena    per layer: x_in f32 [M,D] (residual stream), h1/h2 bf16 [M,D] (LN outputs), qkv bf16 [M,3D], ctx bf16 [M,D],
           lse f32 [B*H,T], x1 f32 [M,D], u/g bf16 [M,4D] (pre/post GELU), LN statistics.  M = B*T token rows.
  CLS tail c_* : compact [B, .] twins of y / x1 / h2 / u / g / x[L] / last and their statistics (and of the backward's
           scratch): what the last layer computes behind its attention when only the head consumes it (see `cls_tail`).
  LayerScale (cfg.layer_scale_init, off by default): folded [L * 5 D^2] operands of the out-projection / FC2 GEMMs (operand dtype)
           + f32 [L * 2D] biases, and per layer an f32 [5 D^2 + 2D] slab of their raw gradients (`_ensure_ls`).
  Patch dropout (cfg.patch_drop_rate, off by default): a training forward keeps K of each sample's N patch tokens, and T above is
           that forward's 1 + K -- the arena is keyed and sized by it, and also holds keep int32 [B, K] (the kept patches,
           ascending), slot int32 [B, N] (its inverse, -1 = dropped) and, with RoPE, cos / sin tables f32 [M, head_dim / 2]
           gathered per token row.  Evaluation arenas keep cfg.seq_len.
  Masked spectrum modelling (cfg.task_type 'mim'): the arena also holds mim_mask int32 [B, N] (non-zero = masked), the block
           selection it is expanded from (mim_keep [B, Kb], mim_slot [B, Nb]), the decoder's output mim_pred f32 [M, P], in bf16
           mode the operand copy mim_last bf16 [M, D] of `last`, and for training mim_dpred [M, P] (operand dtype).  `last` then
           has the GEMMs' zeroed pad rows, the CLS tail is off, and the head is the Linear `decoder` [P, D].
  Register tokens (cfg.num_register_tokens = R, off by default): T = 1 + R + N everywhere above; the projection writes the patch
           rows 1 + R .., vit_embed_finish_reg fills CLS and the R register rows; the average pool and the 'mim' decoder start
           at row 1 + R.  'mim': mim_last / mim_pred / mim_dpred are then compact [B * (N + 1), .] (rows R .. T-1 of each
           sample: the row in front of the patches stands where the loss kernels expect a CLS row and is ignored by them).
  Global average pooling (cfg.global_pool 'avg'): the CLS tail is off; c_last [B, 1, D] holds the mean of the patch rows of
           `last` (vit_token_pool_fwd) and is what the head reads; c_dlast [B, 1, D] takes the head's gradient, which
           vit_token_pool_bwd spreads over every row of dlast.  No other buffer, no parameter, no workspace.
Dropout masks are regenerated from (seed, site) in backward; no mask is stored.

A layer's tail -- out-projection, LN-after, FC1 + GELU, FC2 behind its attention -- is stated once per direction
(`_tail_fwd`, `_tail_bwd`) and runs over a `Rows`: every token row, or the last layer's B CLS rows.
"""
from __future__ import annotations

import collections
import gc
import math
import os
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import _cabi
from . import functional as vf
from ._cabi import ACT_GELU, LOSS_BCE, LOSS_CE, LOSS_L1, LOSS_MSE, LOSS_SOFT_CE, VitError
from .config import ViTConfig, kept_patches, mim_blocks

ALIGN = 8  # elements; keeps every view 32-byte (f32) / 16-byte (bf16) aligned

EMBED = "vit.embeddings."
PROJ = EMBED + "patch_embeddings.projection"
MASK_TOKEN = EMBED + "mask_token"  # task_type 'mim' only (HF ViTForMaskedImageModeling's name)
REGISTERS = EMBED + "register_tokens"  # cfg.num_register_tokens > 0 only (HF Dinov2WithRegisters' name), shape (1, R, D)
# the name stems of one encoder layer's parameters (+ ".weight" / ".bias"): ViTEngine.names[i].fc1 etc.
LayerNames = collections.namedtuple("LayerNames", "ln1 q wo ln2 fc1 fc2")
_LAYER_STEMS = LayerNames("layernorm_before", "attention.attention.query", "attention.output.dense", "layernorm_after",
                          "intermediate.dense", "output.dense")
# LayerScale (cfg.layer_scale_init): the two per-channel factors of a layer and the Linear each one scales, as name stems
LAMBDA = "lambda1"  # HF DINOv2's parameter name: vit.encoder.layer.{i}.layer_scale{1,2}.lambda1
_SCALED = (("layer_scale1", "attention.output.dense"), ("layer_scale2", "output.dense"))
# what a scaled Linear's GEMMs read and write in place of its parameter and gradient slices: the folded operands
# Wf = diag(lambda) W (operand dtype), bf = lambda * b, and the raw gradients of those two (f32)
ScaledLinear = collections.namedtuple("ScaledLinear", "Wf bf dW_raw db_raw")
# ViTEngine._ls; views: name stem -> ScaledLinear, table: vf.LayerScaleTable (entries 2i, 2i + 1 = layer i's two Linears),
# raw_ptrs: the data_ptr of every dW_raw
LayerScaleState = collections.namedtuple("LayerScaleState", "views table raw_ptrs held")
# one slot of ViTEngine._arenas; rows = (the token rows, the CLS rows)
Arena = collections.namedtuple("Arena", "key act tmp Mp rows")


def resolved_loss(task_type: str, loss_name: str) -> Tuple[str, int]:
    """specvit.py:45-55: cls -> CrossEntropy ('ce'); reg -> L1 iff 'l1' in loss_name.lower() else MSE."""
    if task_type == "cls":
        return "ce", LOSS_CE
    if task_type == "reg":
        ln = loss_name or "l2"
        return ln, (LOSS_L1 if "l1" in ln.lower() else LOSS_MSE)
    if task_type == "mim":  # the reconstruction loss is the config's (mim.loss), not the trainer's loss_name
        return "mim", LOSS_MSE
    raise ValueError(f"Unsupported task_type '{task_type}'")


class ParamLayout:
    """name -> (offset, shape) inside the flat buffers; `state_order` is the reference's state_dict order."""

    def __init__(self, cfg: ViTConfig):
        D, P, Fd = cfg.hidden_size, cfg.patch_size, cfg.intermediate_size
        R = int(getattr(cfg, "num_register_tokens", 0) or 0)
        T = cfg.seq_len - R  # the rows of position_embeddings: CLS and the patches; a register takes no position
        self.entries: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        self._span: Dict[str, Tuple[int, int, Tuple[int, ...]]] = {}  # name -> (offset, offset + numel, shape): what view() needs
        self.layer_ranges: List[Tuple[int, int]] = []
        off = 0

        def add(name, shape):
            nonlocal off
            n = math.prod(shape)
            self.entries[name] = (off, tuple(shape))
            self._span[name] = (off, off + n, tuple(shape))
            off += (n + ALIGN - 1) // ALIGN * ALIGN

        e = "vit.embeddings."
        self.embed_start = off
        add(e + "cls_token", (1, 1, D))
        if R > 0:  # directly behind cls_token, inside the embedding block: its bucket, its gradient exchange
            add(e + "register_tokens", (1, R, D))
        if cfg.pos_encoding_type == "learned":
            add(e + "position_embeddings", (1, T, D))
        add(e + "patch_embeddings.projection.weight", (D, P) if cfg.proj_fn == "SW" else (D, 1, P))
        add(e + "patch_embeddings.projection.bias", (D,))
        mim = cfg.task_type == "mim"
        if mim:  # the last entry of the embedding block: its bucket, its gradient exchange
            add(e + "mask_token", (1, 1, D))
        self.embed_end = off
        for i in range(cfg.num_hidden_layers):
            p = f"vit.encoder.layer.{i}."
            start = off
            for n in ("query", "key", "value"):
                add(p + f"attention.attention.{n}.weight", (D, D))
            for n in ("query", "key", "value"):
                add(p + f"attention.attention.{n}.bias", (D,))
            add(p + "attention.output.dense.weight", (D, D))
            add(p + "attention.output.dense.bias", (D,))
            add(p + "intermediate.dense.weight", (Fd, D))
            add(p + "intermediate.dense.bias", (Fd,))
            add(p + "output.dense.weight", (D, Fd))
            add(p + "output.dense.bias", (D,))
            add(p + "layernorm_before.weight", (D,))
            add(p + "layernorm_before.bias", (D,))
            add(p + "layernorm_after.weight", (D,))
            add(p + "layernorm_after.bias", (D,))
            if cfg.layer_scale_init is not None:  # inside the layer's range: its bucket, its lr, its gradient exchange
                for scale, _ in _SCALED:
                    add(p + f"{scale}.{LAMBDA}", (D,))
            self.layer_ranges.append((start, off))
        self.tail_start = off
        add("vit.layernorm.weight", (D,))
        add("vit.layernorm.bias", (D,))
        head = "decoder" if mim else "classifier" if cfg.task_type == "cls" else "regressor"
        self.head = head
        n_out = P if mim else cfg.num_labels  # the decoder maps a token to the P samples of its window
        add(head + ".weight", (n_out, D))
        add(head + ".bias", (n_out,))
        self.n_trainable = off
        add("vit.pooler.dense.weight", (D, D))
        add("vit.pooler.dense.bias", (D,))
        self.n_total = off
        # the order MyViT's state_dict has in the reference (HF module registration order)
        order = [e + "cls_token"]
        if R > 0:
            order.append(e + "register_tokens")
        if cfg.pos_encoding_type == "learned":
            order.append(e + "position_embeddings")
        order += [e + "patch_embeddings.projection.weight", e + "patch_embeddings.projection.bias"]
        if mim:
            order.append(e + "mask_token")
        for i in range(cfg.num_hidden_layers):
            p = f"vit.encoder.layer.{i}."
            for n in ("query", "key", "value"):
                order += [p + f"attention.attention.{n}.weight", p + f"attention.attention.{n}.bias"]
            for n in ("attention.output.dense", "intermediate.dense", "output.dense", "layernorm_before", "layernorm_after"):
                order += [p + n + ".weight", p + n + ".bias"]
            if cfg.layer_scale_init is not None:
                order += [p + f"{scale}.{LAMBDA}" for scale, _ in _SCALED]
        order += ["vit.layernorm.weight", "vit.layernorm.bias", "vit.pooler.dense.weight", "vit.pooler.dense.bias",
                  head + ".weight", head + ".bias"]
        assert sorted(order) == sorted(self.entries)
        self.state_order = order

    def view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        off, end, shape = self._span[name]
        return flat[off:end].view(shape)

    def numel(self, name: str) -> int:
        return self._span[name][1] - self._span[name][0]

    def buckets(self) -> List[Tuple[int, int]]:
        """Gradient buckets in the order backward completes them: tail (final LN + head), layers L-1..0, embeddings."""
        return [(self.tail_start, self.n_trainable)] + list(reversed(self.layer_ranges)) + \
               [(self.embed_start, self.embed_end)]


class Rows:
    """The rows a run of row-wise kernels covers, with their buffers in one arena: every token row (stride 1), or the B rows
    b*T the head consumes (stride T: the last layer's CLS tail).  Strided rows are READ in place from the full tensors (ctx,
    the residual stream) and everything written for them is compact; their dropout masks and the order of their sums are
    those of the rows' ORIGINAL positions k * stride among the full tensor's M (Mp with the GEMMs' zero pad rows) rows."""

    def __init__(self, n: int, stride: int, M: int, Mp: int, act: dict, tmp: dict, c: str, dctx):
        self.n, self.stride, self.M, self.Mp = n, stride, M, Mp  # n: the GEMM row count (Mp for the token rows)
        for k in ("y", "x1", "h2", "u", "g", "mean2", "rstd2", "xL", "last", "meanF", "rstdF"):  # x1 ... rstd2: per layer slot
            setattr(self, k, act[c + k])
        for k in ("dy", "dy2", "dU", "dh", "dlast"):  # training arenas only
            setattr(self, k, tmp.get(c + k))
        self.dx = (tmp.get(c + "dxa"), tmp.get(c + "dxb"))  # the residual gradient's ping-pong pair
        self.dctx = dctx  # where the out-projection's dX goes (its rows k * stride)
        self.last2 = self.last.view(-1, self.last.shape[-1])


class _SideHop:
    """`with engine._on_side as side:` -- the hop onto the engine's second HIP stream: that stream waits for the main stream's
    position, and the block's launches go to it through its own vit_handle (= its own split-K workspace).  `side` is that
    stream, or None with the second stream off: the block then runs where it stands.  One object per engine, not re-entrant."""

    def __init__(self, eng: "ViTEngine"):
        self.eng, self._inner = eng, None

    def __enter__(self):
        eng = self.eng
        side = eng.side_stream
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(eng.flat.device))
            self._inner = inner = (torch.cuda.stream(side), vf.use_handle(eng._side_handle))
            inner[0].__enter__()
            inner[1].__enter__()
        return side

    def __exit__(self, *exc):
        inner, self._inner = self._inner, None
        if inner is not None:
            inner[1].__exit__(*exc)
            inner[0].__exit__(*exc)
        return False


class ViTEngine:
    def __init__(self, cfg: ViTConfig, loss_name: str = ""):
        if cfg.pos_encoding_type == "rope" and (cfg.head_dim % 8) != 0:
            raise ValueError(f"pos_encoding_type='rope' needs head_dim % 8 == 0 here (got {cfg.head_dim}); "
                             f"the reference needs it even (rope.py:28-29)")
        if cfg.pos_encoding_type not in (None, "none", "learned", "rope"):
            raise ValueError(f"Unsupported pos_encoding_type '{cfg.pos_encoding_type}'. "
                             f"Choose from: 'rope', 'learned', 'none', or None")  # embedding.py:74
        if cfg.proj_fn not in ("SW", "C1D", "CNN"):
            raise ValueError(f"Unsupported proj_fn '{cfg.proj_fn}'")  # embedding.py:44
        # what the kernels take, said at construction instead of as a VIT_ERR_UNSUPPORTED in the middle of a step.  The
        # reference's own sweep (configs/sweep.yaml:10-21) reaches head_dim 4 (hidden 32 / 8 heads) and T = 4090 (patch 8,
        # stride 1): both run in both precisions.
        if cfg.hidden_size % cfg.num_attention_heads:
            raise ValueError(f"The hidden size {cfg.hidden_size} is not a multiple of the number of attention heads "
                             f"{cfg.num_attention_heads}.")  # HF ViTSelfAttention.__init__
        if cfg.head_dim % 4 or cfg.head_dim > 128 or cfg.hidden_size % 8 or cfg.patch_size % 8:
            raise ValueError(f"vit_amd kernels need head_dim % 4 == 0 and <= 128, hidden_size % 8 == 0, patch_size % 8 == 0 "
                             f"(got head_dim {cfg.head_dim}, hidden_size {cfg.hidden_size}, patch_size {cfg.patch_size})")
        if not 0.0 <= float(cfg.drop_path_rate) < 1.0:
            raise ValueError(f"drop_path_rate must lie in [0, 1) (got {cfg.drop_path_rate})")
        kept_patches(cfg.num_patches, cfg.patch_drop_rate)  # ValueError outside [0, 1)
        ls = cfg.layer_scale_init
        if ls is not None and (isinstance(ls, bool) or not isinstance(ls, (int, float)) or not math.isfinite(ls) or not ls > 0):
            raise ValueError(f"layer_scale_init must be a finite number > 0, or None for no LayerScale (got {ls!r})")
        reg = getattr(cfg, "num_register_tokens", 0)
        if isinstance(reg, bool) or not isinstance(reg, int) or reg < 0:
            raise ValueError(f"num_register_tokens must be an integer >= 0 (got {reg!r})")
        if reg > 0 and float(cfg.patch_drop_rate) > 0.0:
            raise ValueError(f"num_register_tokens ({reg}) together with patch_drop_rate ({cfg.patch_drop_rate}) is not built yet")
        self.cfg = cfg
        # register tokens: R rows behind CLS; every forward then runs at T = 1 + R + N
        self.reg = int(reg)
        self.loss_name, self.loss_kind = resolved_loss(cfg.task_type, loss_name)
        # masked spectrum modelling (task_type 'mim'): every forward masks a block selection of the patch
        # tokens and the loss is the reconstruction of the masked windows; labels are ignored
        self.mim = cfg.task_type == "mim"
        if self.mim:
            self.loss_kind = LOSS_L1 if cfg.mim_loss == "l1" else LOSS_MSE
        # global average pooling (cfg.global_pool 'avg'): the head reads the mean of the patch rows of the
        # final LayerNorm's output (c_last) instead of its CLS row, so the last layer runs over every row: no CLS tail
        self.set_global_pool(getattr(cfg, "global_pool", "token"))
        # an optional [B, N] device tensor (bool or integer, non-zero = masked) that replaces the drawn mask of the next
        # forwards, like patch_keep does for patch dropout.  None: draw.
        self.mim_mask: Optional[torch.Tensor] = None
        # evaluation forwards draw their masks from a counter of their own (reset_mim_eval), not from the training step
        self.mim_eval_counter = 0
        self._mim_eval_seed, self._reuse_mim_seed = 0, False  # forward(reuse_step=True) repeats the last evaluation-mode draw
        # a classification call whose labels are floating soft targets [B, num_labels] (Mixup / CutMix / label smoothing,
        # vit_amd/mix.py) runs this kind instead, forward and backward; int64 labels run loss_kind as ever (set_soft_loss)
        self.soft_loss_kind = LOSS_SOFT_CE
        self.layout = ParamLayout(cfg)
        self.flat = torch.zeros(self.layout.n_total, dtype=torch.float32)
        self.shadow: Optional[torch.Tensor] = None
        self.grads: Optional[torch.Tensor] = None
        self._shadow_version = -1
        # LayerScale: the folded operands of the scaled Linears, their raw-gradient slabs and the kernels' table (_ensure_ls);
        # None while the feature is off, or nothing is allocated yet
        self.layer_scale = ls is not None
        self._ls: Optional[LayerScaleState] = None
        self._fold_epoch = -1  # the _shadow_epoch the folded operands were made at
        self.names = [LayerNames(*(f"vit.encoder.layer.{i}.{s}" for s in _LAYER_STEMS)) for i in range(cfg.num_hidden_layers)]
        self._arena_key = None
        self._arenas: Dict[bool, Arena] = {}  # train? -> its slot: one arena for training, one for evaluation
        self.act: Dict[str, object] = {}
        self.tmp: Dict[str, torch.Tensor] = {}
        self._Mp = 0  # the current arena's GEMM row count
        self._rows: Optional[Tuple[Rows, Rows]] = None  # the current arena's (token rows, CLS rows)
        self._rope, self._rope_key = None, None
        # patch dropout (cfg.patch_drop_rate): an optional int32 [B, K] device tensor of strictly ascending patch indices per
        # sample that replaces the drawn selection of the next training forwards (reproducing a run; tests).  None: draw.
        self.patch_keep: Optional[torch.Tensor] = None
        self._T = cfg.seq_len  # the sequence length of the forward in hand: 1 + K when it drops patches, cfg.seq_len otherwise
        self.precision = "f32"       # 'f32' (reference default precision='32') | 'bf16' (precision='bf16-mixed')
        self.base_seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        self.step_counter = 0
        self._last = None
        # weight-gradient GEMMs on a second HIP stream (see _dw): None = off
        self.side_stream: Optional[torch.cuda.Stream] = None
        self._side_handle = None
        self._main_handle = None  # this engine's own vit_handle (workspace + launch geometry): see handle()
        self.reserve_cus = -1     # -1 = the process-wide vit_set_option value
        self._side_reads: Dict[int, object] = {}  # data_ptr of a scratch buffer -> event behind its last reader on the side stream
        self._on_side = _SideHop(self)
        # True / False / "auto": the second stream pays when the main stream's GEMMs leave a large part of the chip idle for
        # whole kernels (see _want_side)
        self.overlap_dw = "auto"
        # The head reads one row per image (specvit.py:78-81) and everything behind the last layer's attention is row-wise, so
        # unless the caller asked for hidden states that part of the last layer runs over the B CLS rows only, forward and
        # backward.  False forces the full path (tests; VIT_CLS_TAIL=0: A/B runs of unmodified scripts).
        self.cls_tail = os.environ.get("VIT_CLS_TAIL", "1") != "0"
        self._accum = False  # True inside backward(accumulate=True): the handles' "grad_accumulate" option is on
        self._gen = 0  # bumped by every forward: the activation arena holds ONE forward, backward checks it is still that one
        self.grad_ready_cb: Optional[Callable[[int, int], None]] = None
        # Parameters are views of `flat` with their OWN version counters (nn.Parameter / .data re-pointing do not share
        # the base's), so "were the f32 weights modified since the bf16 shadow was made?" is answered by a signature
        # over the parameters' versions, supplied by the owning module.
        self.version_fn: Callable[[], int] = lambda: self.flat._version

    def set_global_pool(self, mode: str) -> str:
        """`model.global_pool`: 'token' | 'avg'.  Read by every forward; no buffer and no parameter depends on it."""
        if not isinstance(mode, str) or mode not in ("token", "avg") or (mode == "avg" and self.cfg.task_type == "mim"):
            raise ValueError(f"global_pool must be 'token' or 'avg', and 'avg' needs a pooled head (got {mode!r}, task_type "
                             f"{self.cfg.task_type!r})")
        self.cfg.global_pool = mode
        return mode

    @property
    def avg_pool(self) -> bool:
        return getattr(self.cfg, "global_pool", "token") == "avg"

    def set_soft_loss(self, name: str) -> int:
        """`augment.soft_loss`: 'ce' (torch's cross-entropy with probability targets) | 'bce' (binary cross-entropy with logits,
        DeiT-III's head loss) for classification calls with soft targets."""
        if self.loss_kind != LOSS_CE:
            raise ValueError("soft-target losses belong to classification (task_type 'cls')")
        kinds = {"ce": LOSS_SOFT_CE, "bce": LOSS_BCE}
        if name not in kinds:
            raise ValueError(f"soft_loss must be one of {sorted(kinds)}, got {name!r}")
        self.soft_loss_kind = kinds[name]
        return self.soft_loss_kind

    # ------------------------------------------------------------------ precision
    def set_precision(self, precision) -> str:
        """Lightning-style precision strings (basemodule.py:233: `precision=str(train.precision or '32')`).
        '32' -> fp32-class arithmetic: f32 activations, split-bf16 ("x3") MFMA GEMMs, fp32 attention / LayerNorm.
        'bf16-mixed' -> bf16 MFMA operands with fp32 accumulation, residual stream and statistics (the fast path)."""
        ps = str(precision).lower()
        if ps in ("32", "32-true", "fp32", "f32", "float32"):
            mode = "f32"
        elif ps in ("bf16-mixed", "bf16", "bf16-true", "bfloat16"):
            mode = "bf16"
        elif ps in ("16-mixed", "16", "16-true", "fp16"):
            raise ValueError(f"precision '{precision}': fp16 arithmetic is not implemented on this path (it would need loss "
                             f"scaling); use '32' or 'bf16-mixed'")
        else:
            raise ValueError(f"Unsupported precision '{precision}'")
        if mode == "f32" and self.cfg.seq_len > 4096:
            raise ValueError(f"precision '{precision}': the fp32 attention kernels keep a score row in the LDS and take at most "
                             f"4096 tokens (this model has {self.cfg.seq_len}); use 'bf16-mixed'")
        if mode != self.precision:
            self.precision = mode
            self._drop_arenas()
        return mode

    @property
    def adt(self):
        return torch.bfloat16 if self.precision == "bf16" else torch.float32

    # ------------------------------------------------------------------ parameters
    @property
    def device(self):
        return self.flat.device

    def rebind(self, new_flat: torch.Tensor):
        if new_flat.dtype != torch.float32:
            raise VitError("vit_amd keeps master parameters in fp32 (precision '32' / 'bf16-mixed' semantics); "
                           "casting the module to another dtype is not supported")
        self.flat = new_flat.contiguous()
        self.shadow = None
        self.grads = None
        self._shadow_version = -1
        self._drop_arenas()

    def p(self, name: str) -> torch.Tensor:
        return self.layout.view(self.flat, name)

    def _ensure_device_state(self):
        if not self.flat.is_cuda:
            raise VitError("vit_amd runs on an MI355X only: move the model to the GPU first (model.to('cuda')); "
                           "there is no CPU fallback path")
        if self.grads is None:
            self.grads = torch.zeros(self.layout.n_total, dtype=torch.float32, device=self.flat.device)
        if self.precision != "bf16":
            # the x3 GEMMs read the f32 master weights directly; only the folded operands can be stale
            if self.layer_scale:
                ver = self.version_fn()
                if self._shadow_version != ver:
                    self._shadow_version = ver
                self._ensure_folded()
            return
        if self.shadow is None:
            self.shadow = torch.empty(self.layout.n_total, dtype=torch.bfloat16, device=self.flat.device)
            self._shadow_version = -1
        ver = self.version_fn()
        if self._shadow_version != ver:
            vf.cast_f32_bf16(self.flat, self.shadow)
            self._shadow_version = ver
        if self.layer_scale:
            self._ensure_folded()

    # ------------------------------------------------------------------ LayerScale
    # Every write of _shadow_version -- a cast, mark_shadow_fresh() behind a kernel that rewrote flat and shadow through raw
    # pointers, the -1 that invalidates -- counts as one epoch: the folded operands are stale exactly when the shadow is stale or
    # has just been rewritten, so they are refolded when the epoch moved since the last fold.
    _shadow_epoch = 0

    @property
    def _shadow_version(self) -> int:
        return self._shadow_ver

    @_shadow_version.setter
    def _shadow_version(self, ver: int):
        self._shadow_ver = ver
        self._shadow_epoch += 1

    def _ensure_ls(self) -> "LayerScaleState":
        """The LayerScale side buffers, allocated on first use for the current device and precision: folded weights in the GEMM
        operand dtype (L * 5 D^2) and folded biases (L * 2D, f32); per layer a slab of raw gradients (5 D^2 + 2D, f32, zeroed:
        the raw bias gradients must be zero when an accumulating backward begins); the kernels' table, two entries per layer."""
        if self._ls is None:
            c, dev = self.cfg, self.flat.device
            D, Fd, L = c.hidden_size, c.intermediate_size, c.num_hidden_layers
            nw, per = D * D + D * Fd, D * D + D * Fd + 2 * D
            wf = torch.empty(L * nw, dtype=self.adt, device=dev)
            bf = torch.empty(L * 2 * D, dtype=torch.float32, device=dev)
            raw = torch.zeros(L * per, dtype=torch.float32, device=dev)
            views, entries = {}, []
            for i in range(L):
                p, w0, r0 = f"vit.encoder.layer.{i}.", i * nw, i * per
                for k, ((scale, stem), K) in enumerate(zip(_SCALED, (D, Fd))):
                    wo, ro = w0 + k * D * D, r0 + k * D * D  # the out-projection's D x D comes first
                    v = ScaledLinear(Wf=wf[wo:wo + D * K].view(D, K), bf=bf[(2 * i + k) * D:(2 * i + k + 1) * D],
                                     dW_raw=raw[ro:ro + D * K].view(D, K), db_raw=raw[r0 + nw + k * D:r0 + nw + (k + 1) * D])
                    views[p + stem] = v
                    entries.append(dict(W=self.p(p + stem + ".weight"), b=self.p(p + stem + ".bias"),
                                        lam=self.p(p + f"{scale}.{LAMBDA}"), dW=self.g(p + stem + ".weight"),
                                        db=self.g(p + stem + ".bias"), dlam=self.g(p + f"{scale}.{LAMBDA}"), **v._asdict()))
            with vf.use_handle(self.handle()):
                table = vf.layer_scale_table(entries, dev)
            self._ls = LayerScaleState(views, table, frozenset(v.dW_raw.data_ptr() for v in views.values()), (wf, bf, raw))
            self._fold_epoch = -1
        return self._ls

    def fold_layer_scale(self):
        """Wf = diag(lambda) W, bf = lambda * b for every scaled Linear, from the f32 master weights: one launch on the current
        stream (unconditionally: this is also the first node of a captured step)."""
        ls = self._ensure_ls()
        with vf.use_handle(self.handle()):
            vf.layer_scale_fold(ls.table, self.adt)
        self._fold_epoch = self._shadow_epoch

    def _ensure_folded(self):
        if self._ls is None or self._fold_epoch != self._shadow_epoch:
            self.fold_layer_scale()

    def handle(self):
        """This engine's own vit_handle.  Launch geometry (`reserve_cus`) and the split-K / reduction workspace belong to the
        handle, so two engines of one process -- a training and an evaluation model, a sweep's trials -- do not see each
        other's settings (include/vit_amd.h: vit_handle_set_option)."""
        if self._main_handle is None or self._main_handle.device_index != self._device_index():
            self._main_handle = self._new_handle()
        return self._main_handle

    def _device_index(self) -> int:
        dev = self.flat.device
        return dev.index if dev.index is not None else torch.cuda.current_device()

    def _new_handle(self):
        h = _cabi.Handle(self._device_index())
        h.set_option("reserve_cus", self.reserve_cus)
        if self._accum:  # created inside an accumulating backward
            h.set_option("grad_accumulate", 1)
        return h

    def set_reserve_cus(self, n: int):
        """CUs the one-workgroup-per-CU kernels of THIS engine leave to a collective that overlaps them (data-parallel runs);
        -1 = follow the process-wide default."""
        self.reserve_cus = int(n)
        for h in (self._main_handle, self._side_handle):
            if h is not None:
                h.set_option("reserve_cus", self.reserve_cus)

    def mark_shadow_fresh(self):
        self._shadow_version = self.version_fn()

    def w16(self, name: str) -> torch.Tensor:
        """GEMM weight operand: bf16 shadow view, or the f32 master view in f32 mode."""
        return self.layout.view(self.shadow if self.precision == "bf16" else self.flat, name)

    def g(self, name: str) -> torch.Tensor:
        return self.layout.view(self.grads, name)

    # by name stem (self.names[i].fc1, PROJ, ...): W the GEMM operand, b the f32 bias, dW / db their gradient slices.  With
    # LayerScale on, the out-projection and FC2 stems name the folded operands and the raw-gradient slabs instead (the true
    # gradients reach the flat buffer through vit_layer_scale_grad at the end of the layer's backward).
    def _scaled(self, stem: str) -> Optional[ScaledLinear]:
        return None if self._ls is None else self._ls.views.get(stem)

    def W(self, stem: str) -> torch.Tensor:
        v = self._scaled(stem)
        if v is not None:
            return v.Wf
        return self.layout.view(self.shadow if self.precision == "bf16" else self.flat, stem + ".weight")

    def b(self, stem: str) -> torch.Tensor:
        v = self._scaled(stem)
        return self.layout.view(self.flat, stem + ".bias") if v is None else v.bf

    def dW(self, stem: str) -> torch.Tensor:
        v = self._scaled(stem)
        return self.layout.view(self.grads, stem + ".weight") if v is None else v.dW_raw

    def db(self, stem: str) -> torch.Tensor:
        v = self._scaled(stem)
        return self.layout.view(self.grads, stem + ".bias") if v is None else v.db_raw

    def _qkv_w(self, i: int, buf: torch.Tensor):
        """Layer i's adjacent query / key / value weights in `buf` (a flat buffer) as one [3D, D] matrix."""
        off, _ = self.layout.entries[self.names[i].q + ".weight"]
        D = self.cfg.hidden_size
        return buf[off:off + 3 * D * D].view(3 * D, D)

    def _qkv16(self, i: int):
        return self._qkv_w(i, self.shadow if self.precision == "bf16" else self.flat)

    def _qkv_bias(self, i: int, buf: torch.Tensor):
        off, _ = self.layout.entries[self.names[i].q + ".bias"]
        return buf[off:off + 3 * self.cfg.hidden_size]

    # ------------------------------------------------------------------ arena
    def _ensure_arena(self, B: int, train: bool, T: Optional[int] = None):
        """Select (allocating on first use) the activation arena for this batch size.  Training and evaluation forwards keep
        SEPARATE arenas (one slot each): a validation pass between two optimisation steps must not release the training
        arena -- a captured hipGraph (vit_amd/graph.py) replays raw pointers into it, and re-allocating 17 GB per epoch would
        be waste in any case.  A slot is replaced when its batch size, its sequence length or the precision changes.
        `T`: the sequence length the forward runs at -- 1 + K under patch dropout (every buffer is then sized by it, and the arena
        also holds the selection `keep` [B, K], its inverse `slot` [B, N] and, with RoPE, the gathered tables), cfg.seq_len
        otherwise (None)."""
        T = self.cfg.seq_len if T is None else T
        key = (B, train, self.precision, T)
        if self._arena_key == key:
            return
        slot = self._arenas.get(train)
        if slot is not None and slot.key == key:
            self._arena_key, self.act, self.tmp, self._Mp, self._rows = slot
            return
        self.act, self.tmp, self._rows = {}, {}, None
        self._arenas.pop(train, None)  # release the slot's old tensors before allocating their replacement
        # ... and those of models that are no longer referenced: a model and its engine refer to each other, so a dropped model's
        # arena, gradients and workspaces (17 GB at ViT-B; an earlier trial of a sweep, the model before a rebuild) stay allocated
        # until the cycle collector happens to run -- at a moment no caller chooses, possibly in the middle of a step.  An arena is
        # allocated once per batch size, outside the steady state, so this is the place to run it.
        gc.collect()
        c = self.cfg
        dev = self.flat.device
        R = self.reg  # 0 under patch dropout (the two exclude each other)
        D, Fd, H, L, N, P = c.hidden_size, c.intermediate_size, c.num_attention_heads, c.num_hidden_layers, T - 1 - R, c.patch_size
        M = B * T
        Mc = B * (N + 1)  # 'mim': the rows the decoder reads and the loss kernels index (= M without registers)
        # GEMM row count: token rows padded to the 256-row tiles of the ping-pong GEMM core when the widths allow it.
        # Every buffer a GEMM reads or writes is allocated ZEROED with Mp rows and used through its first M rows by
        # everything else (LayerNorm, attention, reducers write real rows only), so pad rows hold zeros or finite
        # bias-only values in the forward tensors and exact zeros in every gradient tensor: dW = dY^T X over Mp rows
        # equals the sum over the M real rows, and bias-gradient column sums likewise.
        Mp = -(-M // 256) * 256 if (D % 256 == 0 and Fd % 256 == 0) else M
        nl = L if train else 1
        f32, b16 = torch.float32, self.adt  # "b16" = the activation/operand dtype of the current precision mode

        def E(shape, dt):
            return torch.empty(shape, dtype=dt, device=dev)

        def G(cols, dt):  # a GEMM operand / result with M real rows (+ zeroed pad rows behind the view)
            return torch.zeros((Mp, cols), dtype=dt, device=dev)[:M]

        def C(cols, dt):  # a CLS-tail buffer, listed per layer slot like its full twin: only the last layer has a tail, so
            return [E((B, cols) if cols else (B,), dt)] * nl  # ONE buffer serves whichever slot that layer has

        act = dict(
            patches=E((B * N, P), b16),
            x=(xs := [E((B, T, D), f32) for _ in range(L + 1)]), xL=xs[L].view(M, D),
            h1=[G(D, b16) for _ in range(nl)], qkv=[G(3 * D, b16) for _ in range(nl)],
            ctx=[G(D, b16) for _ in range(nl)], lse=[E((B * H, T), f32) for _ in range(nl)],
            # bf16 training: the rounding residual of ctx, so the backward's delta sees the context to ~16 bits (vit_amd.h)
            ctx_lo=[E((M, D), b16) if (train and self.precision == "bf16") else None for _ in range(nl)],
            x1=[E((M, D), f32) for _ in range(nl)], h2=[G(D, b16) for _ in range(nl)],
            u=[G(Fd, b16) for _ in range(nl)], g=[G(Fd, b16) for _ in range(nl)],
            mean1=[E((M,), f32) for _ in range(nl)], rstd1=[E((M,), f32) for _ in range(nl)],
            mean2=[E((M,), f32) for _ in range(nl)], rstd2=[E((M,), f32) for _ in range(nl)],
            # 'mim': the decoder's products read every row of `last` (zeroed pad rows, like every GEMM operand)
            last=G(D, f32).view(B, T, D) if self.mim else E((B, T, D), f32), meanF=E((M,), f32), rstdF=E((M,), f32),
            y=G(D, b16),  # dropout(Linear(.)) of the attention-output / FC2 projection, until the next LayerNorm adds it
            # the last layer's CLS tail: one row per image
            c_y=E((B, D), b16), c_x1=C(D, f32), c_h2=C(D, b16), c_u=C(Fd, b16), c_g=C(Fd, b16),
            c_mean2=C(0, f32), c_rstd2=C(0, f32), c_xL=E((B, D), f32), c_last=E((B, 1, D), f32),
            c_meanF=E((B,), f32), c_rstdF=E((B,), f32),
        )
        if T != c.seq_len:  # patch dropout: N above is the kept count K
            i32 = torch.int32
            act.update(keep=E((B, N), i32), slot=E((B, c.num_patches), i32))
            if c.pos_encoding_type == "rope":
                act.update(rope_cos=E((M, c.head_dim // 2), f32), rope_sin=E((M, c.head_dim // 2), f32))
        if self.mim:
            # the patch mask and the block selection it is expanded from; the decoder's operand copy of `last` in bf16 mode
            # (in f32 mode the x3 products read `last` itself); its output, f32 in either mode
            i32 = torch.int32
            nb, kb = mim_blocks(N, c.mim_span, c.mim_mask_ratio)
            # With registers both are compact: rows R .. T-1 of each sample (mim_last then is a copy in either precision).
            act.update(mim_mask=E((B, N), i32), mim_keep=E((B, kb), i32), mim_slot=E((B, nb), i32),
                       mim_last=G(D, b16)[:Mc] if (self.precision == "bf16" or R > 0) else act["last"].view(M, D),
                       mim_pred=E((Mc, P), f32))
        tmp = {}
        if train and self.mim:
            tmp["mim_dpred"] = G(P, b16)[:Mc]
        if train:
            tmp.update(
                dxa=E((M, D), f32), dxb=E((M, D), f32), dy=G(D, b16), dy2=G(D, b16), dU=G(Fd, b16), dh=G(D, b16),
                dqkv=G(3 * D, b16), dctx=G(D, b16), delta=E((B * H, T), f32), dpatch=E((B * N, D), b16),
                # 'mim' with registers: the decoder's dX writes rows R .. T-1 of each sample and nothing else writes dlast, so the
                # CLS and register rows in front keep the zeros of the allocation (the decoder reads none of them)
                dlast=torch.zeros((B, T, D), dtype=f32, device=dev) if (self.mim and R > 0) else E((B, T, D), f32),
                c_dxa=E((B, D), f32), c_dxb=E((B, D), f32), c_dy=E((B, D), b16), c_dy2=E((B, D), b16), c_dU=E((B, Fd), b16),
                c_dh=E((B, D), b16), c_dlast=E((B, 1, D), f32),
                # the CLS tail's dctx: only its rows b*T are ever written, every other row keeps the zero it was allocated
                # with -- the attention backward reads a full [M, D] gradient and no per-step fill is needed.  INVARIANT: the
                # one writer is the out-projection dX of _tail_bwd over the CLS rows, with ldc = T * D (B and T are fixed for
                # the arena's life); anything else that writes this buffer breaks the tail's gradients silently
                # (tests/test_cls_tail_gpu.py poisons the rows in between and checks that nothing rewrites them)
                dctx_cls=G(D, b16),
            )
        rows = (Rows(Mp, 1, M, Mp, act, tmp, "", tmp.get("dctx")), Rows(B, T, M, Mp, act, tmp, "c_", tmp.get("dctx_cls")))
        self._arenas[train] = Arena(key, act, tmp, Mp, rows)
        self._arena_key, self.act, self.tmp, self._Mp, self._rows = self._arenas[train]

    def _drop_arenas(self):
        self._arena_key = None
        self._arenas = {}
        self.act, self.tmp, self._rows = {}, {}, None
        self._ls = None  # the folded operands have the precision's operand dtype and point into flat / grads

    def _rope_tables(self, T: int):
        """Half-width cos / sin tables of RotaryPositionEmbedding (rope.py:36-56), computed on the host by the reference's
        own expression (so the table bits are the reference's) and kept on the device.
        With R register tokens the table of the 1 + N positions is gathered by row on the host: table_R[0] = table[0] and
        table_R[t] = table[max(0, t - R)] for t >= 1 -- CLS keeps position 0, patch n position 1 + n, and a register takes
        position 0, the identity rotation.  Such a table is not linear in t, so it goes to vit_rope_qk (which reads the table
        per row), never to the GEMM's rotating epilogue."""
        c = self.cfg
        R = self.reg
        key = (T, R, c.head_dim, float(c.rope_base), self.flat.device)
        if self._rope_key != key:
            dim = c.head_dim
            inv_freq = 1.0 / (c.rope_base ** (torch.arange(0, dim, 2).float() / dim))
            freqs = torch.outer(torch.arange(T - R).type_as(inv_freq), inv_freq)
            if R > 0:
                freqs = freqs[(torch.arange(T) - R).clamp_(min=0)]
            self._rope = (freqs.cos().contiguous().to(self.flat.device), freqs.sin().contiguous().to(self.flat.device))
            self._rope_key = key
        return self._rope

    # ------------------------------------------------------------------ forward
    def _site(self, layer: int, which: int) -> int:
        """The (seed, site) slots of a step: 0 the embedding dropout; layer i's four are 1 + 4 i + {0: attention probabilities,
        1: attention-output projection, 2: FC2, 3: the layer's two stochastic-depth gates}.  _site(L, 0) = 1 + 4 L, the first
        slot behind the last layer's, belongs to the patch-dropout selection (vit_patch_select; tests/_patchdrop_ref.py)."""
        return 1 + 4 * layer + which

    def kept_count(self, training: bool) -> Optional[int]:
        """Patch dropout: K, the patch tokens per sample a forward keeps -- or None when it keeps them all: not training, rate 0,
        or a rate so small that K == N.  Read on every forward, like the dropout probabilities."""
        c = self.cfg
        K = kept_patches(c.num_patches, c.patch_drop_rate)
        if not training or float(c.patch_drop_rate) <= 0.0 or K >= c.num_patches:
            return None
        return K

    def reset_mim_eval(self):
        """The next evaluation forward draws the first evaluation mask again (MyViT.eval() calls this)."""
        self.mim_eval_counter = 0

    def mim_seed(self, training: bool, step_seed: int) -> int:
        """The seed a 'mim' forward draws its mask from.  Training: the step's seed (the dropout masks' own).  Evaluation: a
        pure function of (base_seed, k), k = the evaluation forwards since reset_mim_eval():
            (base_seed ^ 0x6D696D5F6576616C) + 0x9E3779B97F4A7C15 * (k + 1)   (mod 2^64)
        so every validation epoch sees the masks of the one before, whatever the batches hold."""
        if training:
            return step_seed
        if self._reuse_mim_seed:  # forward(reuse_step=True): the previous evaluation-mode draw, the counter stays
            return self._mim_eval_seed
        k, self.mim_eval_counter = self.mim_eval_counter, self.mim_eval_counter + 1
        self._mim_eval_seed = ((self.base_seed ^ 0x6D696D5F6576616C) + 0x9E3779B97F4A7C15 * (k + 1)) & 0xFFFFFFFFFFFFFFFF
        return self._mim_eval_seed

    def _mim_select(self, B: int, seed: int, training: bool) -> torch.Tensor:
        """This forward's patch mask, int32 [B, N] in the arena: the caller's (`mim_mask`), or drawn -- vit_patch_select keeps Kb
        of the Nb blocks of `mim_span` patches visible, at patch dropout's site (the two features exclude each other), and
        vit_mim_mask expands the selection.  A step record bound to the handle varies the draw per replay of a captured step."""
        c, a = self.cfg, self.act
        N = c.num_patches
        mask, given = a["mim_mask"], self.mim_mask
        if given is not None:
            if not isinstance(given, torch.Tensor) or not given.is_cuda or tuple(given.shape) != (B, N) or given.is_floating_point():
                raise ValueError(f"mim_mask / bool_masked_pos must be a bool or integer [{B}, {N}] device tensor (non-zero = "
                                 f"masked), got {getattr(given, 'dtype', type(given))} {tuple(getattr(given, 'shape', ()))}")
            mask.copy_(given != 0)
            return mask
        nb, kb = mim_blocks(N, c.mim_span, c.mim_mask_ratio)
        vf.patch_select(B, nb, kb, self.mim_seed(training, seed), self._site(c.num_hidden_layers, 0), a["mim_keep"], a["mim_slot"])
        return vf.mim_mask(a["mim_slot"], c.mim_span, mask)

    def path_rates(self, training: bool = True) -> Optional[List[float]]:
        """Stochastic depth: the drop probability of layer i's two residual branches, the usual linear schedule
        torch.linspace(0, drop_path_rate, L) (layer 0 never drops).  None when no branch can drop: not training, or rate 0."""
        rate, L = float(self.cfg.drop_path_rate), self.cfg.num_hidden_layers
        if not training or rate <= 0.0 or L == 0:
            return None
        if not rate < 1.0:
            raise ValueError(f"drop_path_rate must lie in [0, 1) (got {rate})")
        return [float(v) for v in torch.linspace(0, rate, L).tolist()]

    def _path(self, pd: Optional[List[float]], i: int, branch: int, rows_per_sample: Optional[int] = None):
        """The path arguments of layer i's branch (0: attention, 1: MLP) for the LayerNorm passes: (p_i, site, rows per sample,
        branch) with the layer's fourth site, the one dropout leaves free -- or None where nothing can drop.  Rows per sample:
        T in the row space a pass indexes by original row (the backward always; the forward over a stream it reads in place);
        1 where the forward reads a compact stream of one row per sample (the CLS tail's second sum)."""
        if pd is None or i < 0 or pd[i] <= 0.0:
            return None
        return (pd[i], self._site(i, 3), self._T if rows_per_sample is None else rows_per_sample, branch)

    def forward(self, x: torch.Tensor, labels: Optional[torch.Tensor], training: bool, need_grad: bool,
                output_hidden_states: bool = False, output_attentions: bool = False, capture_ctx: Optional[list] = None,
                reuse_step: bool = False):
        """`reuse_step` (the second pass of a sharpness-aware step, vit_amd/sam.py): this forward reads the step seed the
        previous forward used and does not advance `step_counter`, so it draws that forward's dropout masks, drop-path gates,
        patch-dropout selection and `mim` mask again -- the same function of the weights, evaluated at other weights."""
        self._ensure_device_state()
        with vf.use_handle(self.handle()):
            return self._forward(x, labels, training, need_grad, output_hidden_states, output_attentions, capture_ctx, reuse_step)

    def _forward(self, x, labels, training, need_grad, output_hidden_states, output_attentions, capture_ctx, reuse_step=False):
        c = self.cfg
        if x.dim() != 2 or x.shape[1] != c.image_size:
            raise ValueError(f"pixel_values must be [batch, {c.image_size}], got {tuple(x.shape)}")
        if not x.is_cuda:
            raise VitError("pixel_values must live on the GPU")
        K = self.kept_count(training)  # patch dropout: this forward runs at 1 + K tokens (None: at all of them)
        T = c.seq_len if K is None else 1 + K
        if self.precision == "f32" and T > 4096:
            raise ValueError(f"precision '32': the fp32 attention kernels take at most 4096 tokens (this forward has "
                             f"{T}); use train.precision 'bf16-mixed'")
        x = x.contiguous().to(torch.float32)
        B = x.shape[0]
        keep_in = self.patch_keep if K is not None else None
        if keep_in is not None and (not isinstance(keep_in, torch.Tensor) or keep_in.dtype != torch.int32 or not keep_in.is_cuda
                                    or tuple(keep_in.shape) != (B, K)):
            raise ValueError(f"patch_keep must be an int32 [{B}, {K}] device tensor of ascending patch indices per sample, got "
                             f"{getattr(keep_in, 'dtype', type(keep_in))} {tuple(getattr(keep_in, 'shape', ()))}")
        self._gen += 1
        self._T = T
        D, H, L, N, P, S = c.hidden_size, c.num_attention_heads, c.num_hidden_layers, c.num_patches, c.patch_size, c.stride
        dh, M = c.head_dim, B * T
        self._ensure_arena(B, need_grad, T)
        a = self.act
        ph = c.hidden_dropout_prob if training else 0.0
        pa = c.attention_probs_dropout_prob if training else 0.0
        pd = self.path_rates(training)  # read on every forward, like the dropout probabilities
        if reuse_step:
            if self._last is None:
                raise VitError("forward(reuse_step=True) without a preceding forward")
            seed = self._last["seed"]
        else:
            if training:
                self.step_counter += 1
            seed = (self.base_seed + 0x9E3779B97F4A7C15 * self.step_counter) & 0xFFFFFFFFFFFFFFFF
        self._reuse_mim_seed = reuse_step
        scale = dh ** -0.5
        full, cls = self._rows
        # --- embeddings: unfold -> projection (+bias) into token rows 1..N -> CLS / pos-emb / dropout
        x0 = a["x"][0]
        R = self.reg
        pos = self.p(EMBED + "position_embeddings").view(1 + N, D) if c.pos_encoding_type == "learned" else None
        rope = self._rope_tables(c.seq_len) if c.pos_encoding_type == "rope" else None
        # RoPE by a vit_rope_qk pass behind the QKV projection instead of its rotating epilogue: tables that are not linear in the
        # row (patch dropout's per-row gather; the register rows' position 0)
        rope_pass = K is not None or R > 0
        if K is None:
            mask = self._mim_select(B, seed, training) if self.mim else None
            vf.unfold_cast(x, P, S, N, out=a["patches"])  # bf16 or f32 patches, per the arena dtype
            vf.gemm(a["patches"], self.W(PROJ).view(D, P), M=B * N, N=D, K=P, out=x0.view(M, D), bias=self.b(PROJ),
                    row_map=(N, T, 1 + R))
            if R > 0:  # CLS, the register rows, (the mask token,) pos-emb on CLS and patches, dropout on every row
                vf.embed_finish_reg(x0, R, self.p(EMBED + "cls_token").view(D), self.p(REGISTERS).view(R, D), pos, mask,
                                    self.p(MASK_TOKEN).view(D) if mask is not None else None, dropout=(ph, seed, 0))
            elif mask is None:
                vf.embed_finish(x0, self.p(EMBED + "cls_token").view(D), pos, dropout=(ph, seed, 0))
            else:  # a masked patch's projected token gives way to the mask token, in front of pos-emb and dropout
                vf.embed_finish_masked(x0, self.p(EMBED + "cls_token").view(D), mask, self.p(MASK_TOKEN).view(D), pos,
                                       dropout=(ph, seed, 0))
        else:
            # patch dropout: select (or take the caller's selection), then the gather forms of the same three steps; everything
            # behind them is the path below at T = 1 + K.  The selection's site is the first one behind the layers'.
            keep, slot = a["keep"], a["slot"]
            if keep_in is None:
                vf.patch_select(B, N, K, seed, self._site(L, 0), keep, slot)
            else:
                keep.copy_(keep_in)
                vf.patch_slot(keep, slot)
            vf.unfold_gather_cast(x, keep, P, S, N, out=a["patches"])
            vf.gemm(a["patches"], self.W(PROJ).view(D, P), M=B * K, N=D, K=P, out=x0.view(M, D), bias=self.b(PROJ),
                    row_map=(K, T, 1))
            vf.embed_finish_gather(x0, self.p(EMBED + "cls_token").view(D), keep, c.seq_len, pos, dropout=(ph, seed, 0))
            if rope is not None:
                # every token rotates by its ORIGINAL position: per-step tables [B * T, dh / 2], one row per token row, for a
                # vit_rope_qk pass behind the projection (the rotating epilogue takes linear positions only)
                rope = (vf.rows_gather(rope[0], keep, out=a["rope_cos"]), vf.rows_gather(rope[1], keep, out=a["rope_sin"]))

        atts = [] if output_attentions else None
        # the decoder ('mim') and the average pool read every row
        tail = bool(self.cls_tail) and L > 0 and not output_hidden_states and not self.mim and not self.avg_pool
        r = full
        if L == 0:
            self._ln(full.xL, "vit.layernorm", full.last2, full.meanF, full.rstdF)
        else:
            self._ln(x0.view(M, D), self.names[0].ln1, a["h1"][0], a["mean1"][0], a["rstd1"][0])
        for i in range(L):
            j = i if need_grad else 0
            # vit_with_rope.py:58-60: q, k rotated per head before the scores -- inside the projection's epilogue where the
            # kernel has one (f32 values, one rounding), by a vit_rope_qk pass behind it otherwise (the library decides)
            vf.gemm(a["h1"][j], self._qkv16(i), M=full.n, N=3 * D, K=D, out=a["qkv"][j], bias=self._qkv_bias(i, self.flat),
                    rope=None if rope is None or rope_pass else (rope[0], rope[1], T, dh, 2 * D))
            if rope is not None and rope_pass:  # position = row % (the table's rows): M under patch dropout, T with registers
                vf.rope_qk(a["qkv"][j], rope[0], rope[1], M if K is not None else T, H, dh)
            vf.attention_fwd(a["qkv"][j], B, H, T, dh, scale, dropout=(pa, seed, self._site(i, 0)), ctx=a["ctx"][j],
                             lse=a["lse"][j], ctx_lo=a["ctx_lo"][j])
            if output_attentions:
                atts.append(vf.attention_probs(a["qkv"][j], B, H, T, dh, scale))
            if capture_ctx is not None:  # per-layer context for forward hooks on the attention modules
                capture_ctx.append(a["ctx"][j].view(B, T, D).clone())
            if i + 1 < L:  # FC2's output is consumed by the next layer's LN-before
                jn = i + 1 if need_grad else 0
                then = (a["x"][i + 1].view(M, D), self.names[i + 1].ln1, a["h1"][jn], a["mean1"][jn], a["rstd1"][jn])
            else:  # ... or by the final LayerNorm: over the CLS rows alone when only the head consumes it
                r = cls if tail else full
                then = (r.xL, "vit.layernorm", r.last2, r.meanF, r.rstdF)
            self._tail_fwd(r, i, j, a["x"][i].view(M, D), then, ph, seed, need_grad, pd)
        hn = self.layout.head
        kind = self.loss_kind
        if self.mim:
            # pred[b, n, :] = decoder(last[b, 1 + n, :]) over all M rows (the CLS row's output is ignored by the loss), then the
            # reconstruction loss of the masked windows against the signal this forward was given
            # With registers the decoder reads rows R .. T-1 of each sample, gathered (and cast) into the compact mim_last by a
            # strided device copy: N + 1 rows per sample, the loss kernels' layout, whose first row they ignore.
            if R > 0:
                a["mim_last"].view(B, N + 1, D).copy_(full.last[:, R:, :])
            elif self.precision == "bf16":
                vf.cast_f32_bf16(full.last2[:M], a["mim_last"])
            Mc = B * (N + 1)
            pred = vf.gemm(a["mim_last"], self.W(hn), M=Mc, N=P, K=D, out=a["mim_pred"], bias=self.b(hn))
            loss, count = vf.mim_loss_fwd(x, pred, mask, P, S, kind, c.mim_norm_target)
            recon = pred.view(B, N + 1, P)[:, 1:, :]
            self._last = dict(B=B, seed=seed, ph=ph, pa=pa, pd=pd, labels=None, logits=recon, gen=self._gen, grad=need_grad,
                              tail=False, kind=kind, T=T, keep=None, mim=True, mask=mask, count=count, x=x, pred=pred,
                              pool="token")
            hs = [t.clone() for t in a["x"]] if output_hidden_states else None
            return loss, recon, hs, atts
        if labels is not None:
            labels = labels.to(self.flat.device)
            if kind == LOSS_CE and labels.is_floating_point() and tuple(labels.shape) == (B, c.num_labels):
                kind = self.soft_loss_kind  # soft targets: this call's loss, forward and backward
            labels = labels.contiguous().to(torch.int64 if kind == LOSS_CE else torch.float32)
            n_expected = B if kind == LOSS_CE else B * c.num_labels
            if labels.numel() != n_expected:
                raise ValueError(f"labels has {labels.numel()} elements, expected {n_expected}")
        pooled = r.last
        if self.avg_pool:  # the mean of this forward's patch rows (under patch dropout: of the K kept ones), read as [B, 1, D]
            pooled = a["c_last"]
            vf.token_pool_fwd(full.last, 1 + R, out=pooled)
        logits, loss = vf.head_loss_fwd(pooled, self.p(hn + ".weight"), self.p(hn + ".bias"), labels, kind)
        self._last = dict(B=B, seed=seed, ph=ph, pa=pa, pd=pd, labels=labels, logits=logits, gen=self._gen, grad=need_grad,
                          tail=tail, kind=kind, T=T, keep=a["keep"] if K is not None else None, mim=False,
                          pool="avg" if self.avg_pool else "token")
        hs = [t.clone() for t in a["x"]] if output_hidden_states else None
        return loss, logits, hs, atts

    def _tail_fwd(self, r: Rows, i: int, j: int, xin, then, ph: float, seed: int, need_grad: bool, pd=None):
        """Layer i behind its attention, over the rows `r` (activations in layer slot j): out-projection -> LN-after -> FC1 + GELU
        -> FC2 -> `then` = (xsum, name, out, mean, rstd), the LayerNorm that consumes FC2's output (the next layer's LN-before, or
        the final one).
        The two "dropout(Linear(.)) + residual" sums of a layer (HF ViTLayer / ViTOutput) are formed by the LayerNorm that
        consumes them: the projection GEMM writes y = dropout(acc + bias) in the activation dtype, the LayerNorm pass reads the
        f32 stream and y, writes the new stream and its normalised operand (vit_layernorm_fwd_residual).
        Rows of stride T (the CLS rows b*T): ctx and the residual stream `xin` are read in place, everything written is compact,
        and the dropout masks are keyed by the ORIGINAL row b*T so that they are the full path's (and oracle/dropmask.py's)
        bit for bit.
        `pd` (path_rates): with pd[i] > 0 the two sums gate their branch per sample (stochastic depth) inside the same
        LayerNorm passes; the sample of a row is its original row // T, so the CLS rows draw the full path's decisions."""
        c, a, nm = self.cfg, self.act, self.names[i]
        D, Fd, n = c.hidden_size, c.intermediate_size, r.n
        drs = r.stride if r.stride > 1 else 0
        vf.gemm(a["ctx"][j], self.W(nm.wo), M=n, N=D, K=D, lda=r.stride * D, out=r.y, bias=self.b(nm.wo),
                dropout=(ph, seed, self._site(i, 1)), drop_row_stride=drs)
        self._ln_res(xin, r.y, r.x1[j], nm.ln2, r.h2[j], r.mean2[j], r.rstd2[j], x_row_stride=r.stride,
                     path=self._path(pd, i, 0), seed=seed)
        vf.gemm(r.h2[j], self.W(nm.fc1), M=n, N=Fd, K=D, out=r.g[j], bias=self.b(nm.fc1), act=vf.ACT_GELU_GRAD if need_grad
                else ACT_GELU, aux_out=r.u[j] if need_grad else None)  # u holds gelu'(pre-activation) for the backward
        vf.gemm(r.g[j], self.W(nm.fc2), M=n, N=D, K=Fd, out=r.y, bias=self.b(nm.fc2), dropout=(ph, seed, self._site(i, 2)),
                drop_row_stride=drs)
        # x1 is compact over the CLS rows (one row per sample, read with stride 1): the sample of its row b is b
        self._ln_res(r.x1[j], r.y, *then, path=self._path(pd, i, 1, self._T // r.stride), seed=seed)

    def saved_attentions(self):
        """Attention probabilities (before dropout) of every layer of the LAST need_grad forward, from its saved qkv."""
        st, c = self._last, self.cfg
        if st is None or not st["grad"] or st["gen"] != self._gen:
            raise VitError("saved_attentions(): the last forward did not keep per-layer activations")
        with vf.use_handle(self.handle()):
            return [vf.attention_probs(self.act["qkv"][i], st["B"], c.num_attention_heads, st["T"], c.head_dim,
                                       c.head_dim ** -0.5) for i in range(c.num_hidden_layers)]

    def _ln(self, x, name, out, mean, rstd):
        vf.layernorm_fwd(x, self.p(name + ".weight"), self.p(name + ".bias"), self.cfg.layer_norm_eps, out=out,
                         mean=mean, rstd=rstd)

    def _ln_res(self, x, delta, xsum, name, out, mean, rstd, x_row_stride=1, path=None, seed=0):
        # path: the sum gates delta per sample (stochastic depth, vit_layernorm_fwd_residual_path); None = the plain forms
        vf.layernorm_fwd_residual(x, delta, xsum, self.p(name + ".weight"), self.p(name + ".bias"),
                                  self.cfg.layer_norm_eps, out=out, mean=mean, rstd=rstd, x_row_stride=x_row_stride,
                                  path=path, seed=seed)

    # ------------------------------------------------------------------ weight gradients beside the data path
    def _dw(self, r: Rows, dy, x, out, ldx: Optional[int] = None):
        """A weight gradient out[N, K] = dy^T x over the rows `r`: a deterministic split-K GEMM over the token rows, the
        compact product in the full product's summation order over the CLS rows (vf.linear_bwd_dw_rows).  Its only consumer is
        the optimizer at the end of the step, so it is enqueued on a second HIP stream (own vit_handle = own split-K workspace)
        right after its operands are complete and runs beside whatever continues the chain on the main stream.  What that buys:
        the CUs a kernel of the main stream leaves idle (partial rounds of the N = 768 GEMMs, the tail of a LayerNorm pass) get
        dW workgroups -- a GEMM workgroup takes a whole CU (128 KiB of LDS, 2 x 232 of a SIMD's 512 VGPRs), so nothing shares a
        CU with it; measured 0.1-0.2 ms per step.
        Token rows: `dy` is a scratch buffer that a later kernel of this backward overwrites, so an event is recorded behind
        the GEMM and `_before_write(dy)` makes the main stream wait for it before that kernel (one layer later, so the wait is
        normally already satisfied).  CLS rows: no read event is recorded -- c_dy, c_dU and c_dy2 have ONE writer per step
        each, which runs before this call on the main stream, and the next step's writers run behind _join_side; a second
        writer of one of them inside a step would need _before_write like the token rows'."""
        N, K = out.shape
        # a raw-gradient slab of a scaled Linear (LayerScale) is overwritten even inside an accumulating backward: the add into
        # the flat buffer is vit_layer_scale_grad's.  The handle's option is read on the host when the product is planned.
        raw = self._accum and self._ls is not None and out.data_ptr() in self._ls.raw_ptrs
        with self._on_side as side:
            if raw:
                vf._h(out).set_option("grad_accumulate", 0)
            try:
                if r.stride > 1:
                    return vf.linear_bwd_dw_rows(dy, x, out, row_stride=r.stride, full_rows=r.Mp, ldx=ldx)
                vf.gemm(dy, x, M=N, N=K, K=r.n, a_trans=True, b_trans=True, ldb=ldx, out=out, split_k=-1)
            finally:
                if raw:
                    vf._h(out).set_option("grad_accumulate", 1)
            if side is not None:
                ev = torch.cuda.Event()
                ev.record(side)
                self._side_reads[dy.data_ptr()] = ev
        return out

    def _unfold_layer_scale(self, i: int):
        """The end of layer i's backward with LayerScale on: the raw gradients of its two folded Linears become the gradients of
        W, b and lambda in the flat buffer (one launch; it leaves the raw bias gradients zeroed for the next backward).  Issued
        where the layer's weight-gradient GEMMs were, behind them, and in front of the layer's _notify."""
        if self._ls is not None:
            with self._on_side:
                vf.layer_scale_grad(self._ls.table, self._accum, first=2 * i, count=2)

    def _before_write(self, buf):
        """The main stream waits for the second stream's last reader of `buf` (see _dw), if there is one."""
        if self.side_stream is None:
            return
        ev = self._side_reads.pop(buf.data_ptr(), None)
        if ev is not None:
            torch.cuda.current_stream(self.flat.device).wait_event(ev)

    def _join_side(self):
        if self.side_stream is not None:
            torch.cuda.current_stream(self.flat.device).wait_stream(self.side_stream)
            self._side_reads.clear()

    def _notify(self, lo: int, hi: int):
        """Hand grads[lo:hi] to the gradient exchange.  With the second stream on, the collective is enqueued from THAT stream
        (after it has caught up with the main stream's position): the exchange then waits for the weight-gradient GEMMs
        without the main stream having to join them, and the data path of the next layer keeps running."""
        cb = self.grad_ready_cb
        if cb is not None:
            with self._on_side:
                cb(lo, hi)

    def _want_side(self) -> bool:
        """`overlap_dw == "auto"`: second stream iff the balanced grid of this batch's [M, D] x [D, D] products leaves at least
        30 % of the CUs without a workgroup (the dW GEMMs then run on CUs nobody uses).  Measured on MI355X with the half-tile
        tail launch off (r05, tools/stream_rule.sh; the chip is power-limited, so CU-time spent is what counts): ViT-B at B = 64 /
        128 (41 % idle) two streams +3.5 %, ViT-L at B = 32 (43 %) +3.7 %; ViT-B at B = 192 ... 512 (7-23 % idle) within +-0.6 %,
        and at the benchmarked B = 256 one stream wins by 0.5-1 % -- there the hand-off gaps between the streams (0.6 ms per
        step, profiles/r05_a_gaps.txt) cost more than the overlap returns.  Shapes off the 256-aligned core: two streams."""
        if self.overlap_dw != "auto":
            return bool(self.overlap_dw)
        D = self.cfg.hidden_size
        Mp = self._Mp
        if D % 256 or not Mp or Mp % 256:
            return True
        cus = max(1, torch.cuda.get_device_properties(self.flat.device).multi_processor_count - max(0, self.reserve_cus))
        tiles = (Mp // 256) * (D // 256)
        rounds = -(-tiles // cus)
        return -(-tiles // rounds) <= 0.7 * cus

    def _setup_side(self):
        on = self.precision == "bf16" and self._want_side()
        if on and self.side_stream is None:
            self.side_stream = torch.cuda.Stream(device=self.flat.device,
                                                 priority=int(os.environ.get("VIT_SIDE_STREAM_PRIORITY", "0")))
            if self._side_handle is None:
                self._side_handle = self._new_handle()
        elif not on:
            self.side_stream = None

    # ------------------------------------------------------------------ backward
    def _ln_bwd(self, r: Rows, name: str, dy, x, mean, rstd, dres, dx, dyn=None, dbias=None, dropout=vf.NO_DROP,
                dres_row_stride: int = 0, path=None):
        """The backward of LayerNorm `name` over the rows `r`: dx = dres + its input gradient, and the gradients of its weight
        and bias.  With `dyn` it also emits dyn = dropout_mask * dx (activation dtype) and dbias = its column sums: the gradient
        of the Linear output underneath the next "dropout(.) + residual" going down, and that Linear's bias gradient.
        `dres_row_stride = T`: dres alone is compact -- the CLS rows' residual gradient rejoining the token stream.
        `path` (with dyn): that Linear sits in a branch gated per sample -- dyn carries the gate the forward drew
        (vit_layernorm_bwd_path)."""
        vf.layernorm_bwd_rows(dy, x, self.p(name + ".weight"), mean, rstd, dres, dx, self.dW(name), self.db(name), dyn=dyn,
                              dbias=dbias, dropout=dropout, dres_row_stride=dres_row_stride, row_stride=r.stride, full_rows=r.M,
                              path=path)

    def _fc2_dy(self, r: Rows, i: int, ph: float, seed: int, pd=None) -> dict:
        """What the LayerNorm backward that consumes layer i's output emits for that layer's FC2 (_ln_bwd's dyn / dbias):
        r.dy and the FC2 bias gradient, gated like layer i's MLP branch was in the forward (`pd`).  Nothing for i = -1: under
        layer 0's LN-before lie the embeddings."""
        if i < 0:
            return {}
        return dict(dyn=r.dy, dbias=self.db(self.names[i].fc2), dropout=(ph, seed, self._site(i, 2)), path=self._path(pd, i, 1))

    def _tail_bwd(self, r: Rows, i: int, dx, dx_out, ph: float, seed: int, pd=None):
        """Layer i's backward behind its attention, over the rows `r`: from `dx`, the gradient of the layer's output stream
        (r.dy = mask * dx and the FC2 bias gradient came with the LayerNorm backward above), down to r.dctx; the residual
        gradient at the layer's LN-after input goes to `dx_out`.
        Over the CLS rows the weight gradients and bias / LayerNorm parameter sums run over the B rows in the summation order of
        the full-size passes (whose other rows are exact zeros), so they are the full path's bit for bit at T >= 64 (vit_amd.h:
        vit_linear_bwd_dw_rows); the attention-output dX writes its B rows straight into the rows b*T of the otherwise zero
        tmp["dctx_cls"].  Every c_* scratch buffer is written once per step, behind the join of the previous step, so the second
        stream's readers of them record no event and the _before_write calls below find none to wait for.  The row set
        decides two things, both a choice of kernel: the weight-gradient product (_dw) and where the FC1 bias gradient is summed."""
        c, a, nm = self.cfg, self.act, self.names[i]
        D, Fd, n = c.hidden_size, c.intermediate_size, r.n
        strided = r.stride > 1
        # x2 = dropout(g W2^T + b2) + x1
        self._dw(r, r.dy, r.g[i], self.dW(nm.fc2))
        self._before_write(r.dU)
        # the FC1 bias gradient = column sums of dU: in the dX product's epilogue over the token rows, by the pass that sums
        # compact rows in that order behind it over the CLS rows
        vf.gemm(r.dy, self.W(nm.fc2), M=n, N=Fd, K=D, b_trans=True, out=r.dU, act=vf.ACT_MUL_AUX, aux_in=r.u[i],
                colsum_out=None if strided else self.db(nm.fc1))
        if strided:
            vf.colsum_rows(r.dU, self.db(nm.fc1), row_stride=r.stride, full_rows=r.Mp)
        self._dw(r, r.dU, r.h2[i], self.dW(nm.fc1))
        vf.gemm(r.dU, self.W(nm.fc1), M=n, N=D, K=Fd, b_trans=True, out=r.dh)
        # x1 = dropout(ctx Wo^T + bo) + x:  LN2 backward -> dx1, and dy2 = mask * dx1 with dbo
        # this pass writes the OTHER dy buffer: the FC2 weight gradient still reading r.dy keeps running beside it
        self._before_write(r.dy2)
        self._ln_bwd(r, nm.ln2, r.dh, r.x1[i], r.mean2[i], r.rstd2[i], dx, dx_out, dyn=r.dy2, dbias=self.db(nm.wo),
                     dropout=(ph, seed, self._site(i, 1)), path=self._path(pd, i, 0))
        self._dw(r, r.dy2, a["ctx"][i], self.dW(nm.wo), ldx=r.stride * D)
        vf.gemm(r.dy2, self.W(nm.wo), M=n, N=D, K=D, b_trans=True, out=r.dctx, ldc=r.stride * D)

    def _set_accumulate(self, on: bool):
        for h in (self._main_handle, self._side_handle):
            if h is not None:
                h.set_option("grad_accumulate", int(on))

    def backward(self, dloss: torch.Tensor, need_dx: bool = False, gen: Optional[int] = None, accumulate: bool = False):
        """`accumulate=True`: every parameter-gradient slice of self.grads receives old + new instead of new (the
        "grad_accumulate" option of both handles is on for the length of the pass and cleared afterwards, also on error);
        activation gradients are overwritten as ever.  False runs the same kernels with the same arguments as before the option
        existed: nothing is set."""
        with vf.use_handle(self.handle()):
            if not accumulate:
                return self._backward(dloss, need_dx, gen)
            self._accum = True
            try:
                self._set_accumulate(True)
                return self._backward(dloss, need_dx, gen)
            finally:
                self._accum = False
                self._set_accumulate(False)

    def _backward(self, dloss: torch.Tensor, need_dx: bool = False, gen: Optional[int] = None):
        """Fill self.grads (every trainable slice exactly once) for the last forward; calls grad_ready_cb(lo, hi) as
        each bucket of the flat gradient buffer is complete (used to overlap the RCCL all-reduce).  `gen`: the forward this
        backward belongs to (ViTEngine._gen at that time); the arena holds one forward's activations, so a later forward
        (a second loss term, an eval pass, a viz hook) makes them unavailable and that is an error, not a wrong gradient."""
        st = self._last
        if st is None or (st["labels"] is None and not st["mim"]):
            raise VitError("backward without a preceding forward(labels=...)")
        if not st["grad"] or (gen is not None and gen != st["gen"]) or st["gen"] != self._gen:
            raise VitError("backward: the activations of that forward are gone -- another forward ran on this model in "
                           "between (the engine keeps the activations of ONE forward; run backward before the next forward)")
        c = self.cfg
        a, t = self.act, self.tmp
        B, seed, ph, pa, pd = st["B"], st["seed"], st["ph"], st["pa"], st["pd"]  # pd: the forward's path rates
        T, keep = st["T"], st["keep"]  # the forward's sequence length and, under patch dropout, its selection [B, T - 1]
        self._T = T
        R = self.reg  # 0 under patch dropout
        D, H, L, N, P = c.hidden_size, c.num_attention_heads, c.num_hidden_layers, T - 1 - R, c.patch_size  # N: patch rows per sample
        dh, M = c.head_dim, B * T
        scale = dh ** -0.5
        rope, rope_T = None, T
        if c.pos_encoding_type == "rope":  # under patch dropout the forward's gathered tables: one row per token row
            rope, rope_T = (self._rope_tables(T), T) if keep is None else ((a["rope_cos"], a["rope_sin"]), M)
        hn = self.layout.head
        dloss = dloss.reshape(1).to(torch.float32).contiguous()
        full, cls = self._rows
        r = cls if st["tail"] else full  # the rows the backward walks until the last layer's LN-before
        if st["mim"]:
            # dpred (operand dtype; CLS and unmasked rows exact zeros), then the decoder Linear's three products:
            # dlast = dpred W, dW = dpred^T last beside the data path, db = the column sums of dpred
            self._setup_side()
            dpred = t["mim_dpred"]
            vf.mim_loss_bwd(st["x"], st["pred"], st["mask"], st["count"], dloss, P, c.stride, st["kind"], c.mim_norm_target,
                            dpred=dpred)
            # with registers dpred is compact: its row b * (N + 1) + j is the gradient of token row b * T + R + j
            vf.gemm(dpred, self.W(hn), M=B * (N + 1), N=D, K=P, b_trans=True, out=full.dlast.view(M, D),
                    row_map=(N + 1, T, R) if R > 0 else (0, 0, 0))
            self._dw(full, dpred, a["mim_last"], self.dW(hn))
            vf.colsum(dpred, out=self.db(hn), accumulate=self._accum)
        elif st["pool"] == "avg":
            # the head's backward over the pooled rows, then every patch row of dlast takes its sample's share (CLS rows: zeros)
            vf.head_loss_bwd(a["c_last"], self.p(hn + ".weight"), st["logits"], st["labels"], dloss, st["kind"],
                             dlast=t["c_dlast"], dW=self.dW(hn), db=self.db(hn))
            vf.token_pool_bwd(t["c_dlast"], full.dlast, 1 + R)
            self._setup_side()
        else:
            vf.head_loss_bwd(r.last, self.p(hn + ".weight"), st["logits"], st["labels"], dloss, st["kind"], dlast=r.dlast,
                             dW=self.dW(hn), db=self.db(hn))
            self._setup_side()
        dx, spare = r.dx  # the residual gradient and the buffer the next LayerNorm backward writes it to
        self._ln_bwd(r, "vit.layernorm", r.dlast.view(-1, D), r.xL, r.meanF, r.rstdF, None, dx,
                     **self._fc2_dy(r, L - 1, ph, seed, pd))
        self._notify(self.layout.tail_start, self.layout.n_trainable)
        for i in reversed(range(L)):
            self._tail_bwd(r, i, dx, spare, ph, seed, pd)
            dx, spare = spare, dx
            self._before_write(t["dqkv"])
            # the QKV bias gradient = column sums of dqkv: taken by the attention kernels on their way out, unless RoPE
            # sits in between (then after the inverse rotation, by the column-sum kernel)
            vf.attention_bwd(a["qkv"][i], a["ctx"][i], r.dctx, a["lse"][i], B, H, T, dh, scale,
                             dropout=(pa, seed, self._site(i, 0)), dqkv=t["dqkv"], delta=t["delta"],
                             colsum_out=None if rope is not None else self._qkv_bias(i, self.grads), ctx_lo=a["ctx_lo"][i])
            if rope is not None:  # gradient wrt the un-rotated q, k: the inverse rotation
                vf.rope_qk(t["dqkv"], rope[0], rope[1], rope_T, H, dh, inverse=True)
                vf.colsum(t["dqkv"], out=self._qkv_bias(i, self.grads), accumulate=self._accum)
            self._dw(full, t["dqkv"], a["h1"][i], self._qkv_w(i, self.grads))
            vf.gemm(t["dqkv"], self._qkv16(i), M=full.n, N=D, K=3 * D, b_trans=True, out=t["dh"])
            self._before_write(t["dy"])  # the LayerNorm backward below rewrites t["dy"] (read by this layer's FC2 weight gradient)
            # LN1 backward -> dx (input of this layer = output of layer i-1), plus layer i-1's FC2 pieces
            dres, rejoin = dx, 0
            if r is not full:
                # LN1 backward of the last layer: the compact residual gradient joins the token stream at the rows b*T (every
                # other row has none); from here down the gradient is dense and the path is the full one
                rejoin, r = r.stride, full
                dx, spare = full.dx
            self._ln_bwd(full, self.names[i].ln1, t["dh"], a["x"][i].view(M, D), a["mean1"][i], a["rstd1"][i], dres, spare,
                         dres_row_stride=rejoin, **self._fc2_dy(full, i - 1, ph, seed, pd))
            dx, spare = spare, dx
            self._unfold_layer_scale(i)
            self._notify(*self.layout.layer_ranges[i])
        dpos = self.g(EMBED + "position_embeddings").view(-1, D) if c.pos_encoding_type == "learned" else None
        if R > 0:  # the plain and the masked model alike: dcls, dreg, dpos (CLS and patch rows), dmask_token
            mim = st["mim"]
            vf.embed_finish_reg_bwd(dx.view(B, T, D), R, self.g(EMBED + "cls_token").view(D), self.g(REGISTERS).view(R, D), dpos,
                                    st["mask"] if mim else None, self.g(MASK_TOKEN).view(D) if mim else None,
                                    dropout=(ph, seed, 0), dpatch=t["dpatch"])
        elif st["mim"]:  # masked rows: a zero dpatch row, their gradient goes to the mask token
            vf.embed_finish_masked_bwd(dx.view(B, T, D), st["mask"], self.g(EMBED + "cls_token").view(D), self.g(MASK_TOKEN).view(D),
                                       dpos, dropout=(ph, seed, 0), dpatch=t["dpatch"])
        elif keep is None:
            vf.embed_finish_bwd(dx.view(B, T, D), self.g(EMBED + "cls_token").view(D), dpos, dropout=(ph, seed, 0),
                                dpatch=t["dpatch"])  # dtype follows the buffer
        else:  # dpos is summed through the inverse map: rows of patches nobody kept come out zero
            vf.embed_finish_gather_bwd(dx.view(B, T, D), a["slot"], self.g(EMBED + "cls_token").view(D), dpos,
                                       dropout=(ph, seed, 0), dpatch=t["dpatch"])
        vf.colsum(t["dpatch"], out=self.db(PROJ), accumulate=self._accum)
        vf.gemm(t["dpatch"], a["patches"], M=D, N=P, K=B * N, a_trans=True, b_trans=True, out=self.dW(PROJ).view(D, P),
                split_k=-1)
        self._join_side()
        self._notify(self.layout.embed_start, self.layout.embed_end)
        if need_dx:
            # gradient wrt the signal itself (a trainable input preprocessor sits in front): dpatches = dpatch Wp, then the
            # overlap-add that undoes the tokenizer's unfold
            dpat = vf.gemm(t["dpatch"], self.W(PROJ).view(D, P), M=B * N, N=P, K=D, b_trans=True, out_dtype=torch.float32)
            if keep is not None:
                return vf.fold_add_gather(dpat, a["slot"], c.image_size, P, c.stride)
            return vf.fold_add(dpat, B, c.image_size, P, c.stride, N)
        return None
