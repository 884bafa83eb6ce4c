"""Host restatements of register tokens (include/vit_amd_registers.h): the embedding finish and its backward in torch f32 on the
CPU, every batch sum in the header's documented order (`reduce_rows` restates the library's partial-row reducer), and
`registers` -- a context manager under which the UNCHANGED CPU oracle (oracle/refvit.py) runs with R register tokens behind
CLS: `refvit.tokenize` is wrapped to put the registers in front of the patch tokens (the oracle's own `cat` then puts CLS in
front of them), the position tensor gets R zero rows derived from the real one (autograd reaches it), and `refvit.rope_tables`
is swapped for the row-gathered tables (CLS position 0, patch n position 1 + n, a register position 0: no rotation).
"""
import contextlib

import numpy as np
import torch

REG = "vit.embeddings.register_tokens"
POS = "vit.embeddings.position_embeddings"

# (B, R, N, D) of the kernel tests: the smallest case; one register; a ragged 256-column chunk (D = 36); two uneven 16-chunk
# splits of the batch (B = 17: chunks of 2, the last of 1; B = 33: chunks of 3); config C1 (its 4 * 133 partial rows of the mask
# token's sum take the reducer's two-stage form); ViT-B geometry; R = 0, against the existing entry points
SHAPES = [(1, 1, 1, 4), (3, 1, 2, 32), (2, 4, 5, 36), (17, 3, 7, 32), (33, 2, 3, 8), (4, 4, 128, 32), (2, 4, 196, 768),
          (2, 0, 5, 32)]
MASKS = (None, "mixed", "all", "none")


# ------------------------------------------------------------------ the kernels
def chunks(B: int):
    """(c, Y): the batch falls into Y chunks of c consecutive samples."""
    c = -(-B // min(B, 16))
    return c, -(-B // c)


def reduce_rows(rows: torch.Tensor) -> torch.Tensor:
    """S(x_0 .. x_{n-1}) of the header over rows [n, W] (f32): the library's partial-row reducer, add for add."""
    rows = rows.to(torch.float32)
    n, W = rows.shape
    zero = torch.zeros(W, dtype=torch.float32)
    if n > 512:
        G = -(-n // min(32, n // 32))
        folded = []
        for r0 in range(0, n, G):
            r1 = min(n, r0 + G)
            s = zero.clone()
            for j in range(16):
                u = zero.clone()
                for k in range(r0 + j, r1, 16):
                    u = u + rows[k]
                s = s + u
            folded.append(s)
        rows, n = torch.stack(folded), len(folded)
    s = zero.clone()
    for j in range(16):
        a = [zero.clone(), zero.clone()]
        for i, k in enumerate(range(j, n, 16)):
            a[i & 1] = a[i & 1] + rows[k]
        s = s + (a[0] + a[1])
    return s


def make_mask(kind, B: int, N: int, seed: int):
    if kind is None:
        return None
    if kind == "all":
        return torch.ones(B, N, dtype=torch.int32)
    if kind == "none":
        return torch.zeros(B, N, dtype=torch.int32)
    m = torch.from_numpy((np.random.default_rng(seed).random((B, N)) < 0.5).astype(np.int32))
    m.view(-1)[0] = 1  # mixed: at least one masked ...
    if B * N > 1:
        m.view(-1)[-1] = 0  # ... and, where there is room, one visible
    return m * 7  # any non-zero value masks


def multiplier(p: float, seed: int, site: int, B: int, T: int, D: int):
    """The embedding dropout's multiplier [B, T, D] (row b * T + t, registers included), or None at p = 0."""
    from oracle import dropmask as dm

    if p <= 0:
        return None
    return torch.from_numpy(dm.multiplier(dm.drop_cfg(p, seed, site), B * T, D)).view(B, T, D)


def embed_fwd(tok, R, cls, reg, pos=None, mask=None, mask_token=None, mult=None):
    """vit_embed_finish_reg on the host: selects, one f32 add, one f32 multiply."""
    B, T, D = tok.shape
    v = tok.clone()
    v[:, 0] = cls
    if R > 0:
        v[:, 1:1 + R] = reg.view(R, D)
    if mask is not None:
        v[:, 1 + R:] = torch.where(mask[:, :, None] != 0, mask_token.view(1, 1, D), v[:, 1 + R:])
    if pos is not None:
        v[:, 0] = v[:, 0] + pos[0]
        v[:, 1 + R:] = v[:, 1 + R:] + pos[1:]
    return v if mult is None else v * mult


def embed_bwd(dtok, R, mask=None, mult=None, with_pos=True, out_dtype=torch.float32, old=None):
    """vit_embed_finish_reg_bwd on the host: dict(dpatch [B * N, D], dcls [D], dreg [R, D], dpos [1 + N, D] or None, dmt [D] or
    None), every sum in the header's order; `old` (a dict of the same keys) is added last, as `accumulate` does."""
    B, T, D = dtok.shape
    N = T - 1 - R
    g = dtok if mult is None else dtok * mult
    masked = None if mask is None else (mask != 0)[:, :, None]
    dpatch = g[:, 1 + R:] if masked is None else torch.where(masked, torch.zeros((), dtype=torch.float32), g[:, 1 + R:])
    gm = torch.zeros_like(g)
    if masked is not None:
        gm[:, 1 + R:] = torch.where(masked, g[:, 1 + R:], torch.zeros((), dtype=torch.float32))
    c, Y = chunks(B)

    def partial_rows(src):  # [Y, T, D] in slot order: CLS, the patches, the registers
        q = torch.zeros(Y, T, D, dtype=torch.float32)
        for y in range(Y):
            for b in range(y * c, min(B, (y + 1) * c)):
                q[y] = q[y] + src[b]
        return torch.cat([q[:, :1], q[:, 1 + R:], q[:, 1:1 + R]], dim=1)

    q = partial_rows(g)
    over_chunks = lambda t0, t1: reduce_rows(q[:, t0:t1].reshape(Y, -1)).view(t1 - t0, D)
    out = dict(dpatch=dpatch.reshape(B * N, D).to(out_dtype), dcls=over_chunks(0, 1).view(D), dreg=over_chunks(1 + N, T),
               dpos=over_chunks(0, 1 + N) if with_pos else None,
               dmt=None if mask is None else reduce_rows(partial_rows(gm).reshape(Y * T, D)))
    if old is not None:
        for k in ("dcls", "dreg", "dpos", "dmt"):
            if out[k] is not None:
                out[k] = out[k] + old[k].view(out[k].shape)
    return out


def sum_bound(B: int, terms: torch.Tensor) -> torch.Tensor:
    """(B + 2) * 2^-24 * sum |term| over dim 0 (float64): the bound of an f32 sum of B terms in any order."""
    return (B + 2) * 2.0 ** -24 * terms.double().abs().sum(0)


# ------------------------------------------------------------------ the oracle with registers
def gathered_rows(T: int, R: int) -> torch.Tensor:
    """Position of token row t: 0 for CLS and the registers, 1 + n for patch n  (= max(0, t - R))."""
    return (torch.arange(T) - R).clamp(min=0)


def widen_pos(pos: torch.Tensor, R: int) -> torch.Tensor:
    """[1, 1 + N, D] -> [1, 1 + R + N, D] with zero rows for the registers, as a function of `pos` (autograd reaches it)."""
    return torch.cat([pos[:, :1], pos[:, :1].expand(-1, R, -1) * 0, pos[:, 1:]], dim=1)


@contextlib.contextmanager
def registers(params, R: int):
    """Inside the block oracle.refvit.forward runs with params[REG] ([1, R, D]) behind CLS; yields the state dict to hand it
    (position_embeddings widened).  Wraps whatever `refvit.tokenize` is at entry, so it nests INSIDE _mim_ref.masked_tokens."""
    from oracle import refvit

    if R == 0:
        yield params
        return
    tokenize, tables = refvit.tokenize, refvit.rope_tables
    reg = params[REG]

    def tokenize_r(cfg, sd, x):
        tok = tokenize(cfg, sd, x)
        return torch.cat([reg.expand(tok.shape[0], -1, -1).to(tok.dtype), tok], dim=1)

    def tables_r(dim, seq_len, base=10000.0):
        cos, sin = tables(dim, seq_len, base)
        idx = gathered_rows(seq_len, R)
        return cos[idx], sin[idx]

    sd = dict(params)
    if POS in sd:
        sd[POS] = widen_pos(params[POS], R)
    refvit.tokenize, refvit.rope_tables = tokenize_r, tables_r
    try:
        yield sd
    finally:
        refvit.tokenize, refvit.rope_tables = tokenize, tables


def oracle_forward(rc, params, x, labels, R: int, training: bool, masks=None, **kw):
    """refvit.forward with R registers: the head reads row 0 as ever."""
    from oracle import refvit

    with registers(params, R) as sd:
        return refvit.forward(rc, sd, x, labels, training=training, masks=masks, **kw)


def register_values(R: int, D: int, seed: int, std: float = 1.0) -> torch.Tensor:
    return torch.from_numpy((std * np.random.default_rng(seed).standard_normal((1, R, D))).astype(np.float32))
