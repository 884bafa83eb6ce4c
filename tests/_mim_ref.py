"""Host restatements of masked spectrum modelling (include/vit_amd_mim.h), built on tests/_patchdrop_ref.py and the CPU oracle:
the block mask the device draws, the target windows, the reconstruction loss in torch (autograd gives its gradient), and a
context manager under which oracle.refvit.forward embeds `mask_token` in place of the masked patches' projected tokens -- so
that refvit.forward(..., output_hidden_states=True).last_hidden_state, the torch decoder and `loss` below are the oracle of a
whole 'mim' step.  The oracle file itself is not edited.
"""
import contextlib

import numpy as np
import torch

from _patchdrop_ref import select, select_site

MASK_TOKEN = "vit.embeddings.mask_token"


def blocks(N: int, span: int, ratio: float):
    """(Nb, Kb): ceil(N / span) blocks, of which max(1, int(Nb * (1 - ratio))) stay visible (Python doubles, as kept())."""
    Nb = -(-N // span)
    return Nb, max(1, int(Nb * (1.0 - ratio)))


def expand(slot_blocks: np.ndarray, N: int, span: int) -> np.ndarray:
    """int32 [B, N]: mask[b, n] = slot_blocks[b, n // span] < 0."""
    return (slot_blocks[:, np.arange(N) // span] < 0).astype(np.int32)


def mask(B: int, N: int, span: int, ratio: float, seed: int, site: int, keys_xor=None) -> np.ndarray:
    """The mask vit_mim_mask o vit_patch_select(B, Nb, Kb, seed, site) draws: int32 [B, N], 1 = masked."""
    Nb, Kb = blocks(N, span, ratio)
    _, slot = select(B, Nb, Kb, seed, site, keys_xor=keys_xor)
    return expand(slot, N, span)


def targets(x: torch.Tensor, P: int, S: int, N: int, norm: bool = False) -> torch.Tensor:
    """[B, N, P]: window n of sample b is x[b, n * S : n * S + P]; a window that does not fit is all zero (vit_unfold_cast's
    rule).  norm: (t - mean) / sqrt(var + 1e-6) per window, var unbiased (MAE's norm_pix_loss)."""
    B, L = x.shape
    t = torch.zeros(B, N, P, dtype=x.dtype)
    fit = x.unfold(1, P, S)
    n_fit = min(N, fit.shape[1])
    t[:, :n_fit] = fit[:, :n_fit]
    if norm:
        t = (t - t.mean(dim=-1, keepdim=True)) / (t.var(dim=-1, unbiased=True, keepdim=True) + 1e-6).sqrt()
    return t


def loss(pred: torch.Tensor, x: torch.Tensor, m, P: int, S: int, kind: str = "l1", norm: bool = False) -> torch.Tensor:
    """sum over masked (b, n) and p of l(pred - target) / (max(1, m.sum()) * P); pred [B, N, P] (patch rows only)."""
    m = torch.as_tensor(np.asarray(m) if not isinstance(m, torch.Tensor) else m).to(pred.dtype)
    B, N = m.shape
    d = pred - targets(x, P, S, N, norm).to(pred.dtype)
    el = d.abs() if kind == "l1" else d * d
    return (el * m[:, :, None]).sum() / (max(1.0, float(m.sum())) * P)


@contextlib.contextmanager
def masked_tokens(m, mask_token: torch.Tensor):
    """Inside the block oracle.refvit.tokenize returns mask_token [1, 1, D] (or [D]) in the rows of masked patches: the
    substitution sits behind the projection and in front of CLS / position embedding / embedding dropout, as in HF
    ViTEmbeddings.  refvit.forward looks `tokenize` up at call time, so wrapping the module attribute is enough."""
    from oracle import refvit

    orig = refvit.tokenize
    mb = torch.as_tensor(np.asarray(m) if not isinstance(m, torch.Tensor) else m) != 0

    def tokenize(cfg, sd, x):
        tok = orig(cfg, sd, x)
        return torch.where(mb[:, :, None], mask_token.reshape(1, 1, -1).to(tok.dtype), tok)

    refvit.tokenize = tokenize
    try:
        yield
    finally:
        refvit.tokenize = orig


def oracle_step(rc, params, x, m, kind: str, norm: bool, training: bool, masks=None):
    """One 'mim' forward of the oracle: returns (loss, reconstruction [B, N, P], RefOutput with hidden states).  `params`
    holds the encoder's tensors plus MASK_TOKEN and decoder.weight [P, D] / decoder.bias [P] (leaves that want a gradient
    have requires_grad set by the caller)."""
    from oracle import refvit

    with masked_tokens(m, params[MASK_TOKEN]):
        out = refvit.forward(rc, params, x, None, training=training, masks=masks, output_hidden_states=True)
    rec = torch.nn.functional.linear(out.last_hidden_state[:, 1:, :], params["decoder.weight"], params["decoder.bias"])
    return loss(rec, x, m, rc.patch_size, rc.stride, kind, norm), rec, out
