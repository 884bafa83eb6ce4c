"""Host restatements of global average pooling (include/vit_amd_pool.h): the forward in the header's documented order of
summation in numpy f32, the backward, and `oracle_step` -- the CPU oracle's encoder (oracle/refvit.py, not edited) with the
head moved from the CLS row to the mean of the patch rows of its last_hidden_state, gradients by autograd.
"""
import numpy as np
import torch

WAVES = 8  # partial sums per (sample, column): partial w takes rows first + w, first + w + 8, ...

# (B, T, D, first) of the kernel tests, GPU and CPU: one pooled token and one column; two tokens; rows that are not 16-byte
# aligned (D % 4 != 0: the scalar path); first = 0; more rows than partials, uneven among them (n = 128 = 16 per partial at
# T = 129, n = 65 at T = 66: partial 0 holds one row more); the ViT-B and ViT-L/384 rows; D = 36: a ragged 256-column chunk
SHAPES = [(1, 2, 1, 1), (3, 2, 32, 1), (2, 5, 33, 1), (2, 5, 192, 0), (4, 129, 32, 1), (2, 197, 768, 1), (1, 577, 1024, 1),
          (5, 66, 36, 1)]


def inv_count(T: int, first: int) -> np.float32:
    """The kernels' factor: the double 1 / n rounded to f32."""
    return np.float32(1.0 / (T - first))


def pool_fwd(x: np.ndarray, first: int = 1) -> np.ndarray:
    """f32 [B, D]: p_w = x[first + w] + x[first + w + 8] + ... in ascending row order (starting AS its first row, not from
    zero), pooled = (((p_0 + p_1) + ...) + p_{W-1}) * inv, W = min(8, n); every operation an f32 one."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, T, D = x.shape
    n = T - first
    assert 0 <= first < T
    parts = []
    for w in range(min(WAVES, n)):
        acc = x[:, first + w, :].copy()
        for t in range(first + w + WAVES, T, WAVES):
            acc = (acc + x[:, t, :]).astype(np.float32)
        parts.append(acc)
    s = parts[0]
    for p in parts[1:]:
        s = (s + p).astype(np.float32)
    return (s * inv_count(T, first)).astype(np.float32)


def pool_bwd(dpooled: np.ndarray, T: int, first: int = 1) -> np.ndarray:
    """f32 [B, T, D]: dpooled * inv in rows first .. T-1, zeros in front."""
    dpooled = np.ascontiguousarray(dpooled, dtype=np.float32)
    B, D = dpooled.shape
    dx = np.zeros((B, T, D), dtype=np.float32)
    dx[:, first:, :] = (dpooled * inv_count(T, first)).astype(np.float32)[:, None, :]
    return dx


def bound(x: np.ndarray, first: int = 1) -> np.ndarray:
    """[B, D] float64: (n + 2) * 2^-24 * mean_t |x[b, t, d]| over the pooled rows -- the standard bound of an f32 sum of n terms
    in any order ((n - 1) u sum|x|), the rounding of inv and the final multiply, divided by n."""
    n = x.shape[1] - first
    return (n + 2) * 2.0 ** -24 * np.abs(x[:, first:, :].astype(np.float64)).mean(axis=1)


def kernel_input(shape, seed: int, offset: float = 0.0) -> np.ndarray:
    B, T, D, _ = shape
    return (np.random.default_rng(seed).standard_normal((B, T, D)) + offset).astype(np.float32)


def head_loss(rc, logits, labels, soft=None):
    """refvit.loss_fn, or for float targets [B, C] the soft-target CE / BCE of `augment` (torch's own)."""
    from oracle import refvit

    F = torch.nn.functional
    if soft is None:
        return refvit.loss_fn(rc, logits, labels)
    lg = logits.view(-1, rc.num_labels)
    return F.cross_entropy(lg, labels) if soft == "ce" else F.binary_cross_entropy_with_logits(lg, labels)


def oracle_step(rc, params, x, labels, training, masks=None, soft=None, keep_last_grad=False):
    """One forward of the oracle under global_pool 'avg': (loss or None, logits [B, C], RefOutput with hidden states).
    `params`: the state dict (leaves that want a gradient have requires_grad set by the caller).  keep_last_grad: retain the
    gradient of out.last_hidden_state (tests of the pooling's backward read it)."""
    from oracle import refvit

    out = refvit.forward(rc, params, x, None, training=training, masks=masks, output_hidden_states=True)
    if keep_last_grad:
        out.last_hidden_state.retain_grad()
    pooled = out.last_hidden_state[:, 1:].mean(1)
    logits = torch.nn.functional.linear(pooled, params[rc.head_name + ".weight"], params[rc.head_name + ".bias"])
    loss = head_loss(rc, logits, labels, soft) if labels is not None else None
    return loss, logits, out
